// e264_blockdiff.hip -- e264_blockdiff_kernel for gfx950 (MI355X): the block difference maps of a batch of pairs of decoded pictures, both read where they lie in
// HBM (e264hip_frame_blockdiff / e264hip_blockdiff_batch, include/edge264_hip.h).  A translation unit of its own: the code objects of the decoding kernels
// (e264_kernels.hip) and of the digest, preview, diff and histogram kernels do not change with it.  The per-thread body is in e264_blockdiff.h (and run on the
// host by tests/emu/blockdiff_asan.cpp); here are the wrapper and the launcher.
//
// Grid (chunks of the largest pair, pairs): a pair of fewer chunks leaves its other workgroups at once.  Threads share nothing: every record of a map is written
// by exactly one of them, so there is no LDS, no atomic and nothing to clear in front.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_kernels.h"
#include "e264_blockdiff.h"

__global__ __launch_bounds__(BD_NT) void e264_blockdiff_kernel(const E264BlockDiffJob *jobs)
{
	const E264BlockDiffJob &job = jobs[blockIdx.y];
	const uint32_t chunks = job.chunks;
	if (blockIdx.x >= chunks)
		return;
	blockdiff_thread(job.view_a, (const gu8 *)job.base_a, job.slot_bytes_a, job.view_b, (const gu8 *)job.base_b, job.slot_bytes_b, (gu8 *)job.dst, job.k,
		blockIdx.x * BD_NT + threadIdx.x, chunks * BD_NT);
}

// workgroups for a pair: BD_UNITS(k) units per thread over the three planes, one workgroup at least
extern "C" uint32_t e264_blockdiff_chunks(const E264View *view, int k)
{
	uint64_t units = 0;
	for (int p = 0; p < 3; p++)
		units += (uint64_t)((view->plane[p].height + (1u << k) - 1) >> k) * BD_ROW_GROUPS(view->plane[p].width, k);
	const uint64_t per = (uint64_t)BD_NT * BD_UNITS(k);
	const uint64_t chunks = (units + per - 1) / per;
	return chunks ? (uint32_t)chunks : 1u; // (at most 3 * 8192 * 4096 / 1024 < 2^17)
}

extern "C" hipError_t e264_launch_blockdiff(const E264BlockDiffJob *jobs, int n_jobs, uint32_t max_chunks, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_blockdiff_kernel, dim3(max_chunks, n_jobs), dim3(BD_NT), 0, stream, jobs);
	return hipGetLastError();
}
