// e264_diff.h -- e264_diff_kernel's body: the difference record of include/edge264_hip.h (version 1) of two pictures, each read where it lies in its slot (E264View).
// For plane p of A and of B, both w x h samples, i = y * w + x, d_i = |a_i - b_i|:  sad = sum d_i, sse = sum d_i^2, count = the samples with d_i != 0, max = max d_i,
// first = the smallest i with d_i != 0 (E264_DIFF_NONE: none).  Every member is a sum, a max or a min, so a thread returns the record of ITS samples and
// e264_diff.hip combines the threads (wave, workgroup, one set of atomics per workgroup and plane): whatever the split, the same numbers.
// A thread's unit of work is (plane, row y, column group j): the 16 columns 16 j .. 16 j + 15 of row y.  Thread t of nt takes units t, t + nt, ... (y and j kept up
// without a division per unit, as digest_thread and preview_planes do).
//   An INTERIOR unit -- its 16 columns all exist -- loads one 16-byte vector from EACH picture at the row's own address, whatever its alignment (the two pictures'
//   rows generally differ in it; the vector types are 1-byte aligned, as the preview's).  Such a vector lies inside a row of its view, so inside its slot for a view
//   e264hip_view_check has accepted; the body compares both vectors' ends with their slot_bytes all the same and reads a unit that fails byte by byte.
//   Every OTHER unit -- the last columns of a row -- reads single bytes: bytes of the two views only.
// So no byte outside [base_a, base_a + slot_bytes_a) or [base_b, base_b + slot_bytes_b) is read (tests/emu/diff_asan.cpp holds this source to that, compiled for
// the host under the address sanitizer).
// Accumulators: a unit adds at most 16 * 255 to sad and 16 * 255^2 to sse, worked out in 32 bits and added to 64-bit sums UNIT BY UNIT, so no split -- one thread
// doing a whole 65535 x 65535 plane included -- can overflow anything; count, max and first are 32-bit by their definition.
// Arithmetic of an interior unit: the xor of the whole vector is tested first.  Equal vectors (verification, freeze detection: almost all of them) cost nothing
// more.  Differing ones: v_sad_u8 per dword for sad; v_dot4_u32_u8 three times per dword for sum a^2, sum b^2, sum a b and sse = aa + bb - 2 ab; a carry trick and
// a population count for count; v_sad_u8 of the masked bytes for max; a trailing-zero count for first.
// Cost, counted in the assembly (tools/isa_mix.py, the loop's blocks), addresses and loop included: 27 VALU instructions per interior unit whose vectors are equal
// (1.7 per sample: 19 of them the unit's addresses and bounds, 8 the two pointers, the xors and the test) and 117 more for one that differs (144: 9.0 per sample;
// 64 of the 117 are the sixteen bytes' max) against the digest's ~11 per sample.  49 VGPRs, no scratch: eight waves per SIMD.
#ifndef E264_DIFF_H
#define E264_DIFF_H
#include "e264_dev.h"
#include "../../include/edge264_hip.h"

#define DF_NT 256     // threads of a workgroup
#ifndef DF_VECTORS
#define DF_VECTORS 64 // 16-byte loads per thread a picture's chunk count aims at (e264_diff_chunks): 32 units of two loads each, the preview's figure.
                      // Measured for 256 x 1080p pairs, equal pairs / every sample differing: 16 loads 221 / 301 us, 32: 148 / 310, 64: 146 / 301, 128: 150 / 300
                      // (`make variant DEFS=-DDF_VECTORS=..`, profiles/r14_diff.txt)
#endif
#define DF_ROW_GROUPS(w) (((uint32_t)(w) + 15u) >> 4) // column groups of a row of w samples: the width of a plane's grid of units

namespace {

typedef v4u E264_AS_GLOBAL __attribute__((aligned(1))) df_gv4u; // 16 bytes at any address

// what a thread, a wave or a workgroup knows about the three planes.  `first` is E264_DIFF_NONE where count is 0
struct DiffPart { uint64_t sad[3], sse[3]; uint32_t count[3], first[3], max[3]; };

#ifndef E264_HOST_INTRINSICS
E264_DEV uint32_t df_sad4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }         // acc + the four |a_k - b_k| (v_sad_u8)
E264_DEV uint32_t df_dot4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_udot4(a, b, acc, false); }   // acc + the four a_k * b_k (v_dot4_u32_u8)
E264_DEV uint32_t df_popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
E264_DEV uint32_t df_ctz(uint32_t v) { return (uint32_t)__builtin_ctz(v); } // (v != 0)
#else
E264_DEV uint32_t df_sad4(uint32_t a, uint32_t b, uint32_t acc)
{
	for (int k = 0; k < 4; k++) { const uint32_t x = a >> (8 * k) & 255u, y = b >> (8 * k) & 255u; acc += x > y ? x - y : y - x; }
	return acc;
}
E264_DEV uint32_t df_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
	for (int k = 0; k < 4; k++) acc += (a >> (8 * k) & 255u) * (b >> (8 * k) & 255u);
	return acc;
}
E264_DEV uint32_t df_popc(uint32_t v) { uint32_t n = 0; for (; v; v &= v - 1) n++; return n; }
E264_DEV uint32_t df_ctz(uint32_t v) { uint32_t n = 0; for (; !(v & 1u); v >>= 1) n++; return n; }
#endif

// one sample of an edge unit
E264_DEV void diff_sample(const uint32_t a, const uint32_t b, const uint32_t i, uint64_t &sad, uint64_t &sse, uint32_t &count, uint32_t &first, uint32_t &mx)
{
	const uint32_t d = a > b ? a - b : b - a;
	if (d) {
		sad += d; sse += d * d; count++;
		mx = mx > d ? mx : d;
		first = first < i ? first : i;
	}
}

// thread `t` of `nt` (all the threads of this pair's workgroups): the record of its units of the three planes.  Plane p of the two views has one size (the host has checked)
E264_DEV DiffPart diff_thread(const E264View &view_a, const gu8 *base_a, const uint64_t slot_bytes_a, const E264View &view_b, const gu8 *base_b, const uint64_t slot_bytes_b,
	const uint32_t t, const uint32_t nt)
{
	DiffPart r;
#pragma unroll
	for (int p = 0; p < 3; p++) {
		const uint32_t w = view_a.plane[p].width, h = view_a.plane[p].height;
		const uint64_t off_a = view_a.plane[p].offset, stride_a = view_a.plane[p].stride, off_b = view_b.plane[p].offset, stride_b = view_b.plane[p].stride;
		// the plane's units: h rows of nj column groups, unit u = y * nj + j; this thread takes u = t, t + nt, ...
		const uint32_t nj = DF_ROW_GROUPS(w), dy = nt / nj, dj = nt - dy * nj;
		uint32_t y = t / nj, j = t - y * nj;
		uint64_t sad = 0, sse = 0;
		uint32_t count = 0, first = E264_DIFF_NONE, mx = 0;
		while (y < h) {
			const uint64_t at_a = off_a + (uint64_t)y * stride_a + 16u * j, at_b = off_b + (uint64_t)y * stride_b + 16u * j; // the unit's first bytes, from the bases
			const uint32_t i0 = y * w + 16u * j; // ... and its first sample's index in the plane (below 2^32: 65535^2 at most)
			if (16u * j + 16u <= w && at_a + 16u <= slot_bytes_a && at_b + 16u <= slot_bytes_b) {
				const v4u a = *(const df_gv4u *)(base_a + at_a), b = *(const df_gv4u *)(base_b + at_b);
				const v4u x = a ^ b;
				if (x[0] | x[1] | x[2] | x[3]) {
					uint32_t s = 0, aa = 0, bb = 0, ab = 0, k = 0;
#pragma unroll
					for (int c = 3; c >= 0; c--) {
						s = df_sad4(a[c], b[c], s);
						aa = df_dot4(a[c], a[c], aa); bb = df_dot4(b[c], b[c], bb); ab = df_dot4(a[c], b[c], ab); // (16 * 255^2 < 2^20 each)
						// bit 7 of every byte of x that is not 0: the low seven bits carry into it
						count += df_popc((((x[c] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x[c]) & 0x80808080u);
#pragma unroll
						for (int q = 0; q < 4; q++) {
							const uint32_t d = df_sad4(a[c] & 255u << (8 * q), b[c] & 255u << (8 * q), 0u);
							mx = mx > d ? mx : d;
						}
						if (x[c]) k = 4u * c + (df_ctz(x[c]) >> 3); // (c counts down: the lowest differing column stays)
					}
					sad += s; sse += aa + bb - 2u * ab; // sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a b, exact
					first = first < i0 + k ? first : i0 + k;
				}
			} else {
				const uint32_t n = w - 16u * j < 16u ? w - 16u * j : 16u; // (16 j < w: j < nj)
#pragma nounroll
				for (uint32_t c = 0; c < n; c++)
					diff_sample(base_a[at_a + c], base_b[at_b + c], i0 + c, sad, sse, count, first, mx);
			}
			y += dy; j += dj;
			if (j >= nj) { j -= nj; y++; }
		}
		r.sad[p] = sad; r.sse[p] = sse; r.count[p] = count; r.first[p] = first; r.max[p] = mx;
	}
	return r;
}

} // namespace
#endif
