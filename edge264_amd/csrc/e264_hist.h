// e264_hist.h -- e264_hist_kernel's body: the histogram record of include/edge264_hip.h (version 1) of one picture, read where it lies in its slot (E264View).
// For plane p, bin[p][v] = the number of samples of the plane equal to v.  Every bin is a sum, so a thread ADDS the counts of ITS samples to a set of bins it is
// given (`bins`: [3][256] words -- on the device a copy in LDS shared with other threads, updated with LDS atomic adds; on the host plain memory and plain adds)
// and e264_hist.hip adds the workgroups' bins to the picture's record: whatever the split and the order of arrival, the same numbers.
// The walk is e264_diff.h's.  A thread's unit of work is (plane, row y, column group j): the 16 columns 16 j .. 16 j + 15 of row y.  Thread t of nt takes units
// t, t + nt, ... (y and j kept up without a division per unit).
//   An INTERIOR unit -- its 16 columns all exist -- loads one 16-byte vector at the row's own address, whatever its alignment (a 1-byte aligned vector type).
//   Such a vector lies inside a row of its view, so inside its slot for a view e264hip_view_check has accepted; the body compares the vector's end with
//   slot_bytes all the same and reads a unit that fails byte by byte.
//   Every OTHER unit -- the last columns of a row -- reads single bytes: bytes of the view only.
// So no byte outside [base, base + slot_bytes) is read, and no word outside bins[0 .. 767] is touched: a sample is a byte (tests/emu/hist_asan.cpp holds this
// source to both, compiled for the host under the address sanitizer, every plane and every set of bins in a heap block of exactly its size).
//
// A histogram is a scatter with collisions that depend on the data, and the pictures a black-frame detector exists for are its worst case: every lane of a wave
// adding to ONE word of LDS, which the LDS serves one lane after the other.  What an interior unit does about it, cheapest test first:
//   FLAT UNIT      the four dwords equal the first byte broadcast (3 xors folded into an or, one multiply for the broadcast): ONE add of 16.
//   FLAT WAVE      (device only, HS_WAVE_AGG) the lanes of the wave that hold a flat unit all hold the SAME value (a ballot against the first lane's): the first of
//                  them adds 16 x their number, the others nothing.  Black, letterbox bars, flat skies: one LDS atomic per wave and 1024 samples.
//   FLAT DWORD     (HS_DWORD_MERGE) a dword of four equal bytes adds 4 with one atomic.
//   otherwise      one add of 1 per sample.
// The candidates, each a build switch (`make variant DEFS=-D..`), measured for 256 x 1080p pictures per call (profiles/r15_hist.txt item 3; the call's median in ms
// for black pictures / uniform noise / decoded frames; the digest of the same batch takes 0.34 to 0.35):
//   HS_VECTORS 32 / 64 / 128 / 256 / 512      0.213 0.292 0.331 / 0.232 0.321 0.347 / 0.210 0.323 0.358 / 0.285 0.331 0.362 / 0.375 0.411 0.437
//   HS_WAVE_AGG 0 (one copy)                  0.283 0.331 0.357   black + 35 %: the aggregation is KEPT
//   HS_COPIES 4, lane l -> copy l & 3         0.213 0.291 0.292   the fastest on noise and decoded content (0.206 0.289 0.290 with HS_WAVE_AGG 0 beside it)
//   HS_COPIES 4, HS_COPY_WAVE 1               0.211 0.315 0.349   REJECTED: the lanes of one instruction still meet in one word
//   HS_DWORD_MERGE 1                          0.207 0.325 0.323
// Built by default: one copy, flat units, flat-wave aggregation, HS_VECTORS 128 -- the build the GPU suite ran on.  HS_COPIES 4 and HS_VECTORS 32 measured faster
// on noise and decoded content and remain switches until the suite has run on that build (their combination was not measured).
// Read from the assembly, per interior unit: 29 VALU and 1 LDS instruction on the all-equal path, 38 VALU and 16 ds_add_u32 on the general path; 16 VGPRs, no scratch.
#ifndef E264_HIST_H
#define E264_HIST_H
#include "e264_dev.h"
#include "../../include/edge264_hip.h"

#define HS_NT 256      // threads of a workgroup: thread v flushes bin v of each plane
#define HS_BINS 768    // words of one copy of the bins: [3][256]
#ifndef HS_VECTORS
#define HS_VECTORS 128 // 16-byte loads per thread a picture's chunk count aims at (e264_hist_chunks): a unit is one load.  See profiles/r15_hist.txt, item 2
#endif
#ifndef HS_COPIES
#define HS_COPIES 1    // copies of the bins in LDS (a power of two up to 4).  Lane l of a wave adds to copy l & (HS_COPIES - 1) (HS_COPY_WAVE: wave k to copy k)
#endif
#ifndef HS_COPY_WAVE
#define HS_COPY_WAVE 0
#endif
#ifndef HS_WAVE_AGG
#define HS_WAVE_AGG 1
#endif
#ifndef HS_DWORD_MERGE
#define HS_DWORD_MERGE 0
#endif
#define HS_COPY_STRIDE (HS_BINS + (HS_COPIES > 1 ? 1 : 0)) // words from one copy to the next: the same bin of two copies lies in two banks
#define HS_ROW_GROUPS(w) (((uint32_t)(w) + 15u) >> 4)      // column groups of a row of w samples: the width of a plane's grid of units

namespace {

typedef v4u E264_AS_GLOBAL __attribute__((aligned(1))) hs_gv4u; // 16 bytes at any address

// the one primitive the bins are updated through
#ifndef E264_HOST_INTRINSICS
typedef uint32_t __attribute__((address_space(3))) hs_bin_t; // LDS: the adds are ds_add_u32, not flat atomics
E264_DEV void hs_add(hs_bin_t *bin, uint32_t n) { __hip_atomic_fetch_add(bin, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#else
typedef uint32_t hs_bin_t;
E264_DEV void hs_add(hs_bin_t *bin, uint32_t n) { *bin += n; }
#endif

// an interior unit whose sixteen samples are all `v`
E264_DEV void hs_add_flat(hs_bin_t *bins, const uint32_t v)
{
#if HS_WAVE_AGG && !defined(E264_HOST_INTRINSICS)
	// (inside a branch: ballots count the lanes that are here)
	const uint64_t here = __ballot(1), same = __ballot(v == (uint32_t)__builtin_amdgcn_readfirstlane(v));
	if (same == here) {
		if (__builtin_amdgcn_mbcnt_hi((uint32_t)(here >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)here, 0u)) == 0)
			hs_add(bins + v, 16u * (uint32_t)__builtin_popcountll(here)); // (at most 1024)
		return;
	}
#endif
	hs_add(bins + v, 16u);
}

// thread `t` of `nt` (all the threads of this picture's workgroups) adds the counts of its units of the three planes to bins[p * 256 + v]
E264_DEV void hist_thread(const E264View &view, const gu8 *base, const uint64_t slot_bytes, const uint32_t t, const uint32_t nt, hs_bin_t *bins)
{
#pragma unroll
	for (int p = 0; p < 3; p++) {
		const uint32_t w = view.plane[p].width, h = view.plane[p].height;
		const uint64_t off = view.plane[p].offset, stride = view.plane[p].stride;
		hs_bin_t *const b = bins + 256 * p;
		// the plane's units: h rows of nj column groups, unit u = y * nj + j; this thread takes u = t, t + nt, ...
		const uint32_t nj = HS_ROW_GROUPS(w), dy = nt / nj, dj = nt - dy * nj;
		uint32_t y = t / nj, j = t - y * nj;
		while (y < h) {
			const uint64_t at = off + (uint64_t)y * stride + 16u * j; // the unit's first byte, from the base
			if (16u * j + 16u <= w && at + 16u <= slot_bytes) {
				const v4u a = *(const hs_gv4u *)(base + at);
				const uint32_t v = a[0] & 255u, flat = v * 0x01010101u;
				if (((a[0] ^ flat) | (a[1] ^ flat) | (a[2] ^ flat) | (a[3] ^ flat)) == 0) {
					hs_add_flat(b, v);
				} else {
#pragma unroll
					for (int c = 0; c < 4; c++) {
#if HS_DWORD_MERGE
						if (a[c] == (a[c] & 255u) * 0x01010101u) { hs_add(b + (a[c] & 255u), 4u); continue; }
#endif
						hs_add(b + (a[c] & 255u), 1u); hs_add(b + (a[c] >> 8 & 255u), 1u); hs_add(b + (a[c] >> 16 & 255u), 1u); hs_add(b + (a[c] >> 24), 1u);
					}
				}
			} else {
				const uint32_t n = w - 16u * j < 16u ? w - 16u * j : 16u; // (16 j < w: j < nj)
#pragma nounroll
				for (uint32_t c = 0; c < n; c++)
					hs_add(b + base[at + c], 1u);
			}
			y += dy; j += dj;
			if (j >= nj) { j -= nj; y++; }
		}
	}
}

} // namespace
#endif
