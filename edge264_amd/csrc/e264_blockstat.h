// e264_blockstat.h -- e264_blockstat_kernel's body: the block statistics map of include/edge264_hip.h (version 1) of ONE picture, read where it lies in its slot
// (E264View).  For plane p, w x h samples s(y, x), b = 1 << k (k = 3 .. 6), bw = ceil(w / b), bh = ceil(h / b): record (Y, X) = { sum, sumsq, gh, gv } over the
// samples y in [b Y, min(b Y + b, h)), x in [b X, min(b X + b, w)): sum = sum s, sumsq = sum s^2, gh = sum |s(y, x + 1) - s(y, x)| over the block's samples with
// x + 1 < w, gv = sum |s(y + 1, x) - s(y, x)| over those with y + 1 < h.  A pair belongs to the block of its LEFT / TOP sample, also where the other sample lies
// in the next block; a pair that would leave the view does not exist.  The map is Y | Cb | Cr, each plane bh x bw records of 16 bytes, tight.
// A thread's unit of work is (plane, block row Y, column group g): the 16 columns 16 g .. 16 g + 15 of the block row's min(b, h - b Y) rows, e264_blockdiff.h's
// walk.  b = 8: a unit is two records (X = 2 g and, where it exists, 2 g + 1); b = 16: one record; b = 32 / 64: the 2 / 4 ADJACENT lanes that hold a block's pieces
// add their sums across lanes (DPP within a quad, no LDS) and the group's first lane stores the record.  Thread t of nt takes units t, t + nt, ... (Y and g kept up
// without a division per unit).  The left / top rule makes a unit self-contained -- it owns the pairs whose left or top sample it holds -- so halves, lane
// groups and block rows add up with no special case.
//   Reads: a unit whose 16 columns all exist in the view and whose LAST row's vector ends inside slot_bytes reads one 16-byte vector per row at the row's own
//   address, whatever its alignment (the vector type is 1-byte aligned): its own rows and, where y0 + rows < h, ONE more row below the block for the vertical
//   pairs of its last row (the previous row's vector stays in registers).  The sample right of the unit, column c0 + 16 of the same row, is read as one byte where
//   c0 + 16 < w; where the view ends there the sixteenth pair is masked off (the vector's own last byte stands in: a difference of zero).  Every OTHER unit -- the
//   last columns of a row -- reads single bytes of the view: the sample, its right neighbour where x + 1 < w, the one below where y + 1 < h.  So every byte read is
//   a byte of the view and no byte outside [base, base + slot_bytes) is read.
//   Writes: the units partition each plane's records (b >= 16: one record per unit or per group of lanes; b = 8: 16 g < w gives 2 g < bw, and every X < bw has
//   g = X >> 1 with 16 g <= 8 X < w), so every record of the map is stored exactly once, by one 16-byte store, and nothing outside the map: no atomics, nothing
//   cleared in front.  tests/emu/blockstat_asan.cpp holds this source to both, compiled for the host under the address sanitizer.
// Arithmetic, per dword of a row's vector: v_sad_u8 against zero (sum), v_dot4_u32_u8 of the dword with itself (sumsq), v_alignbyte_b32 with the dword that
// follows (the last one: with the byte right of the unit) and v_sad_u8 against it (gh), v_sad_u8 against the same dword of the row below (gv).  The vector's low and
// high eight bytes have accumulators of their own: the two records of b = 8, added at the end for b >= 16.
// The row one sample on could also come from a second, unaligned 16-byte load at + 1; the v_alignbyte_b32 form reads 1 byte more per row instead of 16.  Neither
// form's speed has been measured.
// BS_VGPRS VGPRs, no scratch, no AGPRs, no LDS: eight waves per SIMD.
#ifndef E264_BLOCKSTAT_H
#define E264_BLOCKSTAT_H
#include "e264_dev.h"
#include "../../include/edge264_hip.h"

#define BS_NT 256      // threads of a workgroup
#define BS_VGPRS 49    // the kernel's VGPR count from the cross-compilation for gfx950 (tests/test_blockstat.py holds the build to it); no scratch
#ifndef BS_VECTORS
#define BS_VECTORS 32  // 16-byte loads per thread a picture's chunk count aims at (e264_blockstat_chunks): 4 units at b = 8, 2 at b = 16, one unit above -- the units per
                       // thread e264_blockdiff.h settled on, taken over by analogy: NOT measured for this kernel
#endif
// a block row's column groups: bw * (b / 16) for b >= 32, also where the last block's right pieces lie outside the view (they read nothing), so that a group of
// lanes never straddles two blocks
#define BS_ROW_GROUPS(w, k) ((k) > 4 ? (((uint32_t)(w) + (1u << (k)) - 1u) >> (k)) << ((k) - 4) : ((uint32_t)(w) + 15u) >> 4)
// units per thread at block size 1 << k: a unit is b loads (and one more below it)
#define BS_UNITS(k) (BS_VECTORS >> (k) ? BS_VECTORS >> (k) : 1u)
#ifndef E264_EMU_BLOCKSTAT_STORE
#define E264_EMU_BLOCKSTAT_STORE(at) // what the host build counts (tests/emu/blockstat_asan.cpp): record `at` of the picture's map stored
#endif

namespace {

typedef v4u E264_AS_GLOBAL __attribute__((aligned(1))) bs_gv4u;   // 16 bytes at any address
typedef v4u E264_AS_GLOBAL __attribute__((aligned(16))) bs_grec;  // one E264BlockStat: the map is 16-byte aligned and a record 16 bytes

// 32-bit accumulators of a unit, index 0 for a vector's bytes 0 .. 7 and 1 for its bytes 8 .. 15.  A block holds at most 64 x 64 = 4096 samples and as many
// pairs of each direction: s (sum), h (gh), v (gv) <= 4096 * 255 < 2^21, q (sumsq) <= 4096 * 255^2 < 2^29: nothing wraps, and the same bounds hold for the
// sums over a group of lanes (its units make up ONE block)
struct BsAcc { uint32_t s0, s1, q0, q1, h0, h1, v0, v1; };

#ifndef E264_HOST_INTRINSICS
E264_DEV uint32_t bs_sad4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }       // acc + the four |a_k - b_k| (v_sad_u8)
E264_DEV uint32_t bs_dot4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_udot4(a, b, acc, false); } // acc + the four a_k * b_k (v_dot4_u32_u8)
// x summed over the nl = 2 or 4 adjacent lanes of a group (every lane gets the sum): DPP quad permutes [1,0,3,2] and [2,3,0,1].  All lanes of the GROUP are active
// where this is called (they hold pieces of one block, so they leave the unit loop together; nl = 2 uses only the permute inside a pair, whatever the quad's other pair does).  `partner` is the host build's
template <class F> E264_DEV uint32_t bs_group_add(uint32_t x, const uint32_t nl, const uint32_t, F)
{
	x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xb1, 0xf, 0xf, false);
	if (nl == 4u) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4e, 0xf, 0xf, false);
	return x;
}
#else
E264_DEV uint32_t bs_sad4(uint32_t a, uint32_t b, uint32_t acc)
{
	for (int k = 0; k < 4; k++) { const uint32_t x = a >> (8 * k) & 255u, y = b >> (8 * k) & 255u; acc += x > y ? x - y : y - x; }
	return acc;
}
E264_DEV uint32_t bs_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
	for (int k = 0; k < 4; k++) acc += (a >> (8 * k) & 255u) * (b >> (8 * k) & 255u);
	return acc;
}
// the host's threads run one after the other: what the other lanes of the group hold is worked out here, partner(o, which) being sum `which` of the lane whose
// number differs from this one's by xor o
template <class F> E264_DEV uint32_t bs_group_add(uint32_t x, const uint32_t nl, const uint32_t which, F partner)
{
	for (uint32_t o = 1; o < nl; o++) x += partner(o, which);
	return x;
}
#endif

E264_DEV void bs_store(gu8 *dst, const uint32_t at, const uint32_t sum, const uint32_t sumsq, const uint32_t gh, const uint32_t gv)
{
	*(bs_grec *)(dst + 16u * (uint64_t)at) = (v4u){sum, sumsq, gh, gv};
	E264_EMU_BLOCKSTAT_STORE(at);
}

// the row one sample on from its own vector a and, in nb's low byte, the sample right of the vector (a's own last byte where there is none: no pair)
E264_DEV v4u bs_shift(const v4u a, const uint32_t nb)
{
	return (v4u){v_alignbyte(a[1], a[0], 1u), v_alignbyte(a[2], a[1], 1u), v_alignbyte(a[3], a[2], 1u), v_alignbyte(nb, a[3], 1u)};
}

// one row's vector a, the same row one sample on (sh) and the row below it (a itself where there is none: no pair)
E264_DEV void bs_row(BsAcc &r, const v4u a, const v4u sh, const v4u below)
{
	const uint32_t r0 = sh[0], r1 = sh[1], r2 = sh[2], r3 = sh[3];
	r.s0 = bs_sad4(a[0], 0u, r.s0); r.s0 = bs_sad4(a[1], 0u, r.s0);
	r.s1 = bs_sad4(a[2], 0u, r.s1); r.s1 = bs_sad4(a[3], 0u, r.s1);
	r.q0 = bs_dot4(a[0], a[0], r.q0); r.q0 = bs_dot4(a[1], a[1], r.q0);
	r.q1 = bs_dot4(a[2], a[2], r.q1); r.q1 = bs_dot4(a[3], a[3], r.q1);
	r.h0 = bs_sad4(a[0], r0, r.h0); r.h0 = bs_sad4(a[1], r1, r.h0); // (pair 7 = bytes 7 and 8: the left sample's half)
	r.h1 = bs_sad4(a[2], r2, r.h1); r.h1 = bs_sad4(a[3], r3, r.h1);
	r.v0 = bs_sad4(a[0], below[0], r.v0); r.v0 = bs_sad4(a[1], below[1], r.v0);
	r.v1 = bs_sad4(a[2], below[2], r.v1); r.v1 = bs_sad4(a[3], below[3], r.v1);
}

// a unit: `rows` rows of the 16 columns from c0 (at: the first row's first byte, from base); `below`: the view has a row under the unit's last; columns from w on
// do not exist
E264_DEV BsAcc bs_unit(const gu8 *base, uint64_t at, const uint64_t stride, const uint64_t slot_bytes, const uint32_t rows, const bool below, const uint32_t c0, const uint32_t w)
{
	BsAcc r = {0, 0, 0, 0, 0, 0, 0, 0};
	if (c0 >= w) return r; // (a piece of a lane group right of the view)
	const uint32_t nload = rows + (below ? 1u : 0u); // rows read: the unit's and the one below it
	if (c0 + 16u <= w && at + (uint64_t)(nload - 1u) * stride + 16u <= slot_bytes) { // (the last vector read ends inside the slot: so do all before it)
		const bool more = c0 + 16u < w;
		v4u cur = *(const bs_gv4u *)(base + at);
#pragma nounroll
		for (uint32_t y = 0; y < rows; y++, at += stride) {
			v4u nxt = cur;
			if (y + 1u < nload) nxt = *(const bs_gv4u *)(base + at + stride);
			const v4u sh = bs_shift(cur, more ? (uint32_t)base[at + 16u] : cur[3] >> 24); // (column c0 + 16 < w of this row: a byte of the view)
			bs_row(r, cur, sh, nxt);
			cur = nxt;
		}
	} else {
		const uint32_t n = w - c0 < 16u ? w - c0 : 16u;
#pragma nounroll
		for (uint32_t y = 0; y < rows; y++, at += stride) {
			const bool under = y + 1u < nload;
#pragma nounroll
			for (uint32_t i = 0; i < n; i++) {
				const uint32_t s = base[at + i];
				uint32_t dh = 0, dv = 0;
				if (c0 + i + 1u < w) { const uint32_t t = base[at + i + 1u]; dh = s > t ? s - t : t - s; }
				if (under) { const uint32_t t = base[at + stride + i]; dv = s > t ? s - t : t - s; }
				if (i < 8u) { r.s0 += s; r.q0 += s * s; r.h0 += dh; r.v0 += dv; }
				else { r.s1 += s; r.q1 += s * s; r.h1 += dh; r.v1 += dv; }
			}
		}
	}
	return r;
}

// thread `t` of `nt` (all the threads of this picture's workgroups, a multiple of 4): its units of the three planes.  k is 3 .. 6 and the view is one
// e264hip_view_check accepts for slot_bytes (the host has checked); dst is the picture's map, 16-byte aligned
E264_DEV void blockstat_thread(const E264View &view, const gu8 *base, const uint64_t slot_bytes, gu8 *dst, const uint32_t k, const uint32_t t, const uint32_t nt)
{
	const uint32_t b = 1u << k;
	const uint32_t gl = k > 4u ? k - 4u : 0u, nl = 1u << gl; // log2 of the lanes that share a block, and their number
	uint32_t po = 0; // the plane's first record in the map
#pragma unroll
	for (int p = 0; p < 3; p++) {
		const uint32_t w = view.plane[p].width, h = view.plane[p].height;
		const uint64_t off = view.plane[p].offset, stride = view.plane[p].stride;
		const uint32_t bw = (w + b - 1u) >> k, bh = (h + b - 1u) >> k;
		// the plane's units: bh block rows of ng column groups, unit u = Y * ng + g; this thread takes u = t, t + nt, ...
		const uint32_t ng = BS_ROW_GROUPS(w, k), dY = nt / ng, dg = nt - dY * ng;
		uint32_t Y = t / ng, g = t - Y * ng;
		while (Y < bh) {
			const uint32_t y0 = Y << k, rows = h - y0 < b ? h - y0 : b; // (b Y < h: Y < bh)
			const bool below = y0 + rows < h;
			const uint64_t row = off + (uint64_t)y0 * stride; // the block row's first byte, from the base
			const BsAcc r = bs_unit(base, row + (g << 4), stride, slot_bytes, rows, below, g << 4, w);
			if (k == 3u) { // two records: the unit's columns 0 .. 7 and, where the view has them, 8 .. 15
				bs_store(dst, po + Y * bw + 2u * g, r.s0, r.q0, r.h0, r.v0);
				if (2u * g + 1u < bw)
					bs_store(dst, po + Y * bw + 2u * g + 1u, r.s1, r.q1, r.h1, r.v1);
			} else if (nl == 1u)
				bs_store(dst, po + Y * bw + g, r.s0 + r.s1, r.q0 + r.q1, r.h0 + r.h1, r.v0 + r.v1);
			else { // the nl lanes t & ~(nl - 1) .. hold the pieces g & ~(nl - 1) .. of block g >> gl (nt and ng are multiples of nl): they are all here
				auto partner = [&](const uint32_t o, const uint32_t which) {
					const uint32_t go = g ^ o;
					const BsAcc q = bs_unit(base, row + (go << 4), stride, slot_bytes, rows, below, go << 4, w);
					return which == 0u ? q.s0 + q.s1 : which == 1u ? q.q0 + q.q1 : which == 2u ? q.h0 + q.h1 : q.v0 + q.v1;
				};
				const uint32_t s = bs_group_add(r.s0 + r.s1, nl, 0u, partner), q = bs_group_add(r.q0 + r.q1, nl, 1u, partner);
				const uint32_t gh = bs_group_add(r.h0 + r.h1, nl, 2u, partner), gv = bs_group_add(r.v0 + r.v1, nl, 3u, partner);
				if (!(g & (nl - 1u)))
					bs_store(dst, po + Y * bw + (g >> gl), s, q, gh, gv);
			}
			Y += dY; g += dg;
			if (g >= ng) { g -= ng; Y++; }
		}
		po += bw * bh;
	}
}

} // namespace
#endif
