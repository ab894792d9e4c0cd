// e264_digest.hip -- e264_digest_kernel for gfx950 (MI355X): the digests of a batch of decoded pictures, read where they lie in HBM
// (e264hip_frame_digest / e264hip_digest_batch, include/edge264_hip.h).  A translation unit of its own: the code objects of the decoding kernels
// (e264_kernels.hip) do not change with it.  The per-thread body is in e264_digest.h (and run on the host by tests/emu/digest_asan.cpp); here
// are the reduction and the launcher.
//
// Grid (chunks of the largest picture, pictures): a picture of fewer chunks leaves its other workgroups at once.  Every thread sums its share of the
// three planes, the wave adds its lanes up (shuffles), the workgroup its waves (LDS), and one thread per plane adds the workgroup's sum to the
// picture's result with a 64-bit integer atomic: integer addition commutes, so the result does not depend on the order the workgroups arrive in.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_kernels.h"
#include "e264_digest.h"

__global__ __launch_bounds__(DG_NT) void e264_digest_kernel(const E264DigestJob *jobs, unsigned long long *out)
{
	__shared__ unsigned long long part[DG_NT / 64][3];
	const E264DigestJob &job = jobs[blockIdx.y];
	const uint32_t chunks = job.chunks;
	if (blockIdx.x >= chunks)
		return;
	const DigestSums s = digest_thread(job.view, (const gu8 *)job.base, job.slot_bytes, blockIdx.x * DG_NT + threadIdx.x, chunks * DG_NT);
#pragma unroll
	for (int p = 0; p < 3; p++) {
		unsigned long long v = s.d[p];
#pragma unroll
		for (int o = 32; o; o >>= 1)
			v += __shfl_xor(v, o);
		if ((threadIdx.x & 63) == 0)
			part[threadIdx.x >> 6][p] = v;
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		unsigned long long v = 0;
#pragma unroll
		for (int k = 0; k < DG_NT / 64; k++)
			v += part[k][threadIdx.x];
		atomicAdd(&out[3 * blockIdx.y + threadIdx.x], v);
	}
}

// workgroups for a picture: DG_UNITS vectors per thread over its three planes, one workgroup at least
extern "C" uint32_t e264_digest_chunks(const E264View *view)
{
	uint64_t units = 0;
	for (int p = 0; p < 3; p++)
		units += (uint64_t)view->plane[p].height * DG_ROW_VECTORS(view->plane[p].width);
	const uint64_t per = (uint64_t)DG_NT * DG_UNITS;
	const uint64_t chunks = (units + per - 1) / per;
	return chunks ? (uint32_t)chunks : 1u; // (at most 3 * 65535 * 4097 / 2048 < 2^19)
}

extern "C" hipError_t e264_launch_digest(const E264DigestJob *jobs, int n_jobs, uint32_t max_chunks, uint64_t *out, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_digest_kernel, dim3(max_chunks, n_jobs), dim3(DG_NT), 0, stream, jobs, (unsigned long long *)out);
	return hipGetLastError();
}
