// e264_preview.hip -- e264_preview_kernel for gfx950 (MI355X): the reduced previews (box filter by 2, 4 or 8) of a batch of decoded pictures, read where they
// lie in HBM (e264hip_frame_preview / e264hip_preview_batch, include/edge264_hip.h).  A translation unit of its own: the code objects of the decoding kernels
// (e264_kernels.hip) and of the digest kernel (e264_digest.hip) do not change with it.  The per-thread body is in e264_preview.h (and run on the host by
// tests/emu/preview_asan.cpp); here are the wrapper and the launcher.
//
// Grid (chunks of the largest picture, pictures): a picture of fewer chunks leaves its other workgroups at once.  Threads share nothing: every byte of a
// preview is written by exactly one of them, so there is no LDS, no atomic and nothing to clear in front.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_kernels.h"
#include "e264_preview.h"

__global__ __launch_bounds__(PV_NT) void e264_preview_kernel(const E264PreviewJob *jobs)
{
	const E264PreviewJob &job = jobs[blockIdx.y];
	const uint32_t chunks = job.chunks;
	if (blockIdx.x >= chunks)
		return;
	preview_thread(job.view, (const gu8 *)job.base, job.slot_bytes, (gu8 *)job.dst, job.k, blockIdx.x * PV_NT + threadIdx.x, chunks * PV_NT);
}

// workgroups for a picture: PV_VECTORS 16-byte loads per thread (a unit is 1 << k of them) over its three planes, one workgroup at least
extern "C" uint32_t e264_preview_chunks(const E264View *view, int k)
{
	uint64_t units = 0;
	for (int p = 0; p < 3; p++)
		units += (uint64_t)((view->plane[p].height + (1u << k) - 1) >> k) * PV_ROW_GROUPS(view->plane[p].width);
	const uint64_t per = (uint64_t)PV_NT * (PV_VECTORS >> k);
	const uint64_t chunks = (units + per - 1) / per;
	return chunks ? (uint32_t)chunks : 1u; // (at most 3 * 32768 * 4096 / 256 < 2^21)
}

extern "C" hipError_t e264_launch_preview(const E264PreviewJob *jobs, int n_jobs, uint32_t max_chunks, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_preview_kernel, dim3(max_chunks, n_jobs), dim3(PV_NT), 0, stream, jobs);
	return hipGetLastError();
}
