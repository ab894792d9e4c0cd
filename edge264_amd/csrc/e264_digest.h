// e264_digest.h -- e264_digest_kernel's body: the digest of include/edge264_hip.h (version 1) of one picture, read where it lies in its slot (E264View).
// For a plane of w x h samples, i = y * w + x:  D = sum of (s_i + 1) * (fmix32(i) | 1)  mod 2^64 -- a commutative sum, so a thread returns the sum over ITS samples
// and e264_digest.hip adds the threads up (wave, workgroup, one 64-bit atomic per workgroup and plane): whatever the split, the same bits.
// A thread's unit of work is one ALIGNED 16-byte vector of a row (one global_load_dwordx4): the bytes of it that lie left of the row's first sample or right of
// its last are masked out of the sum.  Aligned means aligned in the slot, whose base is a device allocation: a vector that starts inside the slot never
// starts before it, and the one vector that may END behind it -- base + slot_bytes falls inside it: the last row of a plane that ends the slot, the tight layout's
// Cr -- is read byte by byte, the view's bytes only.  So with a view that e264hip_view_check has accepted for slot_bytes, no byte outside
// [base, base + slot_bytes) is read (tests/emu/digest_asan.cpp holds this source to that, compiled for the host under the address sanitizer).
// Cost: ~11 VALU instructions per sample (two multiplies and three shift-xors of the hash, the or, the byte's extraction, one 64-bit multiply-add), from the
// source; the loads are 1 byte per sample.  Not tuned beyond the vector loads and the on-chip reduction.
#ifndef E264_DIGEST_H
#define E264_DIGEST_H
#include "e264_dev.h"

#define DG_NT 256   // threads of a workgroup
#define DG_UNITS 8  // 16-byte vectors per thread a picture's chunk count aims at (e264_digest_chunks)
// vectors a row of w samples can touch at the worst alignment of its first byte (15 bytes into a vector): the width of a plane's grid of units
#define DG_ROW_VECTORS(w) ((((uint32_t)(w) + 14u) >> 4) + 1u)

namespace {

struct DigestSums { uint64_t d[3]; }; // Y, Cb, Cr

E264_DEV uint32_t digest_fmix32(uint32_t h)
{
	h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
	return h;
}
E264_DEV uint64_t digest_term(uint32_t s, uint32_t i) { return (uint64_t)(s + 1u) * (digest_fmix32(i) | 1u); } // (v_mad_u64_u32 with the running sum)

// thread `t` of `nt` (all the threads of this picture's workgroups): its share of the three sums
E264_DEV DigestSums digest_thread(const E264View &view, const gu8 *base, const uint64_t slot_bytes, const uint32_t t, const uint32_t nt)
{
	DigestSums r;
#pragma unroll
	for (int p = 0; p < 3; p++) {
		const uint32_t w = view.plane[p].width, h = view.plane[p].height;
		const uint64_t off = view.plane[p].offset, stride = view.plane[p].stride;
		// the plane's units: h rows of nv vectors, unit u = y * nv + j; this thread takes u = t, t + nt, ... (y and j kept up without a division per unit)
		const uint32_t nv = DG_ROW_VECTORS(w), dy = nt / nv, dj = nt - dy * nv;
		uint32_t y = t / nv, j = t - y * nv;
		uint64_t acc = 0;
		while (y < h) {
			const uint64_t row = off + (uint64_t)y * stride; // the row's first sample, in bytes from base
			const uint64_t v = (row & ~(uint64_t)15) + 16u * j; // this unit's vector
			if (v < row + w) { // (a row that starts well aligned, or is short, does not reach its last vectors)
				const uint32_t x0 = (uint32_t)(v - row); // the column of the vector's first byte: "negative" (it wraps) left of the row
				const uint32_t i0 = y * w + x0;       // ... and its index in the plane: below 2^32 wherever x is a column
				if (v + 16u <= slot_bytes) {
					const v4u q = *(const gv4u *)(base + v);
#pragma unroll
					for (uint32_t b = 0; b < 16; b++)
						if (x0 + b < w) acc += digest_term(q[b >> 2] >> (8 * (b & 3)) & 255u, i0 + b);
				} else { // the slot ends inside this vector: single bytes, those of the view only (all of them lie in the slot: e264hip_view_check)
					for (uint32_t b = 0; b < 16; b++)
						if (x0 + b < w) acc += digest_term(base[v + b], i0 + b);
				}
			}
			y += dy; j += dj;
			if (j >= nv) { j -= nv; y++; }
		}
		r.d[p] = acc;
	}
	return r;
}

} // namespace
#endif
