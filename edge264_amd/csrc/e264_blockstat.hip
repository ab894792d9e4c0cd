// e264_blockstat.hip -- e264_blockstat_kernel for gfx950 (MI355X): the block statistics maps of a batch of decoded pictures, each read where it lies in HBM
// (e264hip_frame_blockstat / e264hip_blockstat_batch, include/edge264_hip.h).  A translation unit of its own: the code objects of the decoding kernels
// (e264_kernels.hip) and of the digest, preview, diff, histogram and block difference kernels do not change with it.  The per-thread body is in
// e264_blockstat.h (and run on the host by tests/emu/blockstat_asan.cpp); here are the wrapper and the launcher.
//
// Grid (chunks of the largest picture, pictures): a picture of fewer chunks leaves its other workgroups at once.  Threads share nothing: every record of a map
// is written by exactly one of them, so there is no LDS, no atomic and nothing to clear in front.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_kernels.h"
#include "e264_blockstat.h"

__global__ __launch_bounds__(BS_NT) void e264_blockstat_kernel(const E264BlockStatJob *jobs)
{
	const E264BlockStatJob &job = jobs[blockIdx.y];
	const uint32_t chunks = job.chunks;
	if (blockIdx.x >= chunks)
		return;
	blockstat_thread(job.view, (const gu8 *)job.base, job.slot_bytes, (gu8 *)job.dst, job.k, blockIdx.x * BS_NT + threadIdx.x, chunks * BS_NT);
}

// workgroups for a picture: BS_UNITS(k) units per thread over the three planes, one workgroup at least
extern "C" uint32_t e264_blockstat_chunks(const E264View *view, int k)
{
	uint64_t units = 0;
	for (int p = 0; p < 3; p++)
		units += (uint64_t)((view->plane[p].height + (1u << k) - 1) >> k) * BS_ROW_GROUPS(view->plane[p].width, k);
	const uint64_t per = (uint64_t)BS_NT * BS_UNITS(k);
	const uint64_t chunks = (units + per - 1) / per;
	return chunks ? (uint32_t)chunks : 1u; // (at most 3 * 8192 * 4096 / 256 < 2^19)
}

extern "C" hipError_t e264_launch_blockstat(const E264BlockStatJob *jobs, int n_jobs, uint32_t max_chunks, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_blockstat_kernel, dim3(max_chunks, n_jobs), dim3(BS_NT), 0, stream, jobs);
	return hipGetLastError();
}
