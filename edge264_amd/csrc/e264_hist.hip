// e264_hist.hip -- e264_hist_kernel for gfx950 (MI355X): the histogram records of a batch of decoded pictures, each read where it lies in HBM
// (e264hip_frame_hist / e264hip_hist_batch, include/edge264_hip.h).  A translation unit of its own: the code objects of the decoding kernels
// (e264_kernels.hip), of the digest, the preview and the diff kernel do not change with it.  The per-thread body is in e264_hist.h (and run on the host by
// tests/emu/hist_asan.cpp); here are the bins in LDS, the flush and the launcher.
//
// Grid (chunks of the largest picture, pictures): a picture of fewer chunks leaves its other workgroups at once.  A workgroup clears its HS_COPIES copies of the
// bins ([3][256] words each) in LDS, every thread adds its share of the three planes to its copy with LDS atomics (e264_hist.h), and behind a barrier thread v adds
// bin v of each plane, summed over the copies, to the picture's record with ONE 32-bit atomic -- only where it is not zero, so a workgroup issues at most 768
// global atomics, and as many as it met distinct (plane, value) pairs: 3 for a black picture.  The record starts as zeros (one clear in front of the kernel, as for
// the diff); sums commute, so it does not depend on the order the workgroups arrive in, and there is no "last workgroup" protocol.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_kernels.h"
#include "e264_hist.h"

static_assert(HS_NT == 256, "thread v flushes bin v");
static_assert(HS_COPIES == 1 || HS_COPIES == 2 || HS_COPIES == 4, "HS_COPIES is 1, 2 or 4");

__global__ __launch_bounds__(HS_NT) void e264_hist_kernel(const E264HistJob *jobs, E264Hist *out)
{
	__shared__ uint32_t bins[HS_COPIES * HS_COPY_STRIDE];
	const E264HistJob &job = jobs[blockIdx.y];
	const uint32_t chunks = job.chunks;
	if (blockIdx.x >= chunks)
		return;
	for (uint32_t i = threadIdx.x; i < HS_COPIES * HS_COPY_STRIDE; i += HS_NT)
		bins[i] = 0;
	__syncthreads();
	const uint32_t copy = HS_COPY_WAVE ? (threadIdx.x >> 6) & (HS_COPIES - 1) : threadIdx.x & (HS_COPIES - 1);
	hist_thread(job.view, (const gu8 *)job.base, job.slot_bytes, blockIdx.x * HS_NT + threadIdx.x, chunks * HS_NT, (hs_bin_t *)bins + copy * HS_COPY_STRIDE);
	__syncthreads();
	uint32_t *r = &out[blockIdx.y].bin[0][0];
#pragma unroll
	for (int p = 0; p < 3; p++) {
		uint32_t n = 0;
#pragma unroll
		for (int c = 0; c < HS_COPIES; c++)
			n += bins[c * HS_COPY_STRIDE + 256 * p + threadIdx.x];
		if (n)
			atomicAdd(r + 256 * p + threadIdx.x, n);
	}
}

// workgroups for a picture: HS_VECTORS 16-byte loads (units) per thread over the three planes, one workgroup at least
extern "C" uint32_t e264_hist_chunks(const E264View *view)
{
	uint64_t units = 0;
	for (int p = 0; p < 3; p++)
		units += (uint64_t)view->plane[p].height * HS_ROW_GROUPS(view->plane[p].width);
	const uint64_t per = (uint64_t)HS_NT * HS_VECTORS;
	const uint64_t chunks = (units + per - 1) / per;
	return chunks ? (uint32_t)chunks : 1u; // (at most 3 * 65535 * 4096 / 256 < 2^22 for HS_VECTORS 1)
}

extern "C" hipError_t e264_launch_hist(const E264HistJob *jobs, int n_jobs, uint32_t max_chunks, E264Hist *out, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_hist_kernel, dim3(max_chunks, n_jobs), dim3(HS_NT), 0, stream, jobs, out);
	return hipGetLastError();
}
