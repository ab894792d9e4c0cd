// e264_diff.hip -- e264_diff_kernel for gfx950 (MI355X): the difference records of a batch of pairs of decoded pictures, both read where they lie in HBM
// (e264hip_frame_diff / e264hip_diff_batch, include/edge264_hip.h).  A translation unit of its own: the code objects of the decoding kernels
// (e264_kernels.hip), of the digest kernel and of the preview kernel do not change with it.  The per-thread body is in e264_diff.h (and run on the host by
// tests/emu/diff_asan.cpp); here are the reduction and the launcher.
//
// Grid (chunks of the largest pair, pairs): a pair of fewer chunks leaves its other workgroups at once.  Every thread works out the record of its share of the
// three planes, the wave combines its lanes (shuffles), the workgroup its waves (LDS), and one thread per plane adds the workgroup's record to the pair's with
// one set of atomics: 64-bit adds for sad and sse, a 32-bit add for count, a max for max and -- the results start as ZEROS, one clear serves them -- a max for
// ~first, which the host turns round after the copy (~E264_DIFF_NONE = 0: "none" is what the clear leaves).  Sums, max and min commute, so the record does not
// depend on the order the workgroups arrive in.  A workgroup that found no difference in a plane has nothing to add and issues no atomic for it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_kernels.h"
#include "e264_diff.h"

__global__ __launch_bounds__(DF_NT) void e264_diff_kernel(const E264DiffJob *jobs, E264Diff *out)
{
	__shared__ unsigned long long part_sad[DF_NT / 64][3], part_sse[DF_NT / 64][3];
	__shared__ uint32_t part_count[DF_NT / 64][3], part_nfirst[DF_NT / 64][3], part_max[DF_NT / 64][3];
	const E264DiffJob &job = jobs[blockIdx.y];
	const uint32_t chunks = job.chunks;
	if (blockIdx.x >= chunks)
		return;
	const DiffPart s = diff_thread(job.view_a, (const gu8 *)job.base_a, job.slot_bytes_a, job.view_b, (const gu8 *)job.base_b, job.slot_bytes_b,
		blockIdx.x * DF_NT + threadIdx.x, chunks * DF_NT);
#pragma unroll
	for (int p = 0; p < 3; p++) {
		unsigned long long sad = s.sad[p], sse = s.sse[p];
		uint32_t count = s.count[p], nfirst = ~s.first[p], mx = s.max[p];
		if (__any(count != 0)) { // (most waves of a verification or a freeze detector: nothing to combine)
#pragma unroll
			for (int o = 32; o; o >>= 1) {
				sad += __shfl_xor(sad, o); sse += __shfl_xor(sse, o); count += __shfl_xor(count, o);
				nfirst = max(nfirst, (uint32_t)__shfl_xor(nfirst, o)); mx = max(mx, (uint32_t)__shfl_xor(mx, o));
			}
		}
		if ((threadIdx.x & 63) == 0) {
			const int k = threadIdx.x >> 6;
			part_sad[k][p] = sad; part_sse[k][p] = sse; part_count[k][p] = count; part_nfirst[k][p] = nfirst; part_max[k][p] = mx;
		}
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		const int p = threadIdx.x;
		unsigned long long sad = 0, sse = 0;
		uint32_t count = 0, nfirst = 0, mx = 0;
#pragma unroll
		for (int k = 0; k < DF_NT / 64; k++) {
			sad += part_sad[k][p]; sse += part_sse[k][p]; count += part_count[k][p];
			nfirst = max(nfirst, part_nfirst[k][p]); mx = max(mx, part_max[k][p]);
		}
		if (count) {
			E264PlaneDiff *r = &out[blockIdx.y].plane[p];
			atomicAdd((unsigned long long *)&r->sad, sad);
			atomicAdd((unsigned long long *)&r->sse, sse);
			atomicAdd(&r->count, count);
			atomicMax(&r->first, nfirst); // (~first: see above)
			atomicMax(&r->max, mx);
		}
	}
}

// workgroups for a pair: DF_VECTORS 16-byte loads per thread (a unit is two of them) over the three planes, one workgroup at least
extern "C" uint32_t e264_diff_chunks(const E264View *view)
{
	uint64_t units = 0;
	for (int p = 0; p < 3; p++)
		units += (uint64_t)view->plane[p].height * DF_ROW_GROUPS(view->plane[p].width);
	const uint64_t per = (uint64_t)DF_NT * (DF_VECTORS / 2);
	const uint64_t chunks = (units + per - 1) / per;
	return chunks ? (uint32_t)chunks : 1u; // (at most 3 * 65535 * 4096 / 8192 < 2^17)
}

extern "C" hipError_t e264_launch_diff(const E264DiffJob *jobs, int n_jobs, uint32_t max_chunks, E264Diff *out, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_diff_kernel, dim3(max_chunks, n_jobs), dim3(DF_NT), 0, stream, jobs, out);
	return hipGetLastError();
}
