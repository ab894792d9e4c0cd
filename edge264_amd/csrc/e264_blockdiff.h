// e264_blockdiff.h -- e264_blockdiff_kernel's body: the block difference map of include/edge264_hip.h (version 1) of two pictures, each read where it lies in its
// slot (E264View).  For plane p of A and of B, both w x h samples, b = 1 << k (k = 3 .. 6), bw = ceil(w / b), bh = ceil(h / b): record (Y, X) = { sad, sse } over the
// samples y in [b Y, min(b Y + b, h)), x in [b X, min(b X + b, w)); samples outside the view do not count.  The map is Y | Cb | Cr, each plane bh x bw records, tight.
// A thread's unit of work is (plane, block row Y, column group g): the G = max(16, b) columns G g .. G g + G - 1 of the block row's min(b, h - b Y) rows of BOTH
// pictures.  b = 8: a unit is two records (X = 2 g and, where it exists, 2 g + 1) from one 16-byte vector per row; b = 16: one record from one vector per row;
// b = 32 / 64: one record from two / four vectors per row (BD_LANE_GROUPS=0; the shipped form for these two sizes is below).  Thread t of nt takes units t, t + nt, ... (Y and g kept up without a division per unit, as diff_thread
// does), so consecutive threads take consecutive column groups.
//   Reads are the diff's: a 16-byte vector whose columns all exist in the view is loaded from EACH picture at the row's own address, whatever its alignment (the
//   vector type is 1-byte aligned); both vectors' ends are compared with their slot_bytes all the same and a vector that fails is read byte by byte.  Every OTHER
//   piece -- the last columns of a row -- is read as single bytes: bytes of the two views only.  So no byte outside [base_a, base_a + slot_bytes_a) or
//   [base_b, base_b + slot_bytes_b) is read.
//   Writes: the units partition each plane's records (b >= 16: ceil(w / G) = bw groups, one record each; b = 8: 16 g < w gives 2 g < bw, and every X < bw has
//   g = X >> 1 with 16 g <= 8 X < w), so every record of the map is stored exactly once, by one 8-byte store, and nothing outside the map: no atomics, nothing
//   cleared in front.  tests/emu/blockdiff_asan.cpp holds this source to both, compiled for the host under the address sanitizer.
// Arithmetic: the xor of the two vectors is tested first; an equal vector adds nothing.  A differing one: v_sad_u8 per dword for sad, v_dot4_u32_u8 three times
// per dword for sum a^2 + sum b^2 (one chain) and sum a b; sse = (sum a^2 + sum b^2) - 2 sum a b at the unit's end.  The vector's low and high eight bytes have
// accumulators of their own: the two records of b = 8, added at the end for b >= 16.
// BD_LANE_GROUPS=1, the shipped build, splits a block of 32 / 64 over 2 / 4 adjacent lanes (below): the same source, one cross-lane add per sum.
// Cost, counted in the assembly (tools/isa_mix.py, the loop's blocks): profiles/r16_blockdiff.txt.  BD_VGPRS VGPRs, no scratch: eight waves per SIMD.
#ifndef E264_BLOCKDIFF_H
#define E264_BLOCKDIFF_H
#include "e264_dev.h"
#include "../../include/edge264_hip.h"

#define BD_NT 256      // threads of a workgroup
#define BD_VGPRS 50    // the kernel's VGPR count from the cross-compilation for gfx950 (tests/test_blockdiff.py holds the build to it); no scratch
#ifndef BD_VECTORS
#define BD_VECTORS 64  // 16-byte loads per thread a pair's chunk count aims at (e264_blockdiff_chunks): 4 units at b = 8, 2 at b = 16, one unit above
#endif
#ifndef BD_LANE_GROUPS
#define BD_LANE_GROUPS 1 // the decomposition for b = 32 / 64.  1: a unit is 16 columns of a block's rows whatever b, and the 2 / 4 ADJACENT lanes that hold a block's pieces
                         // add their sums across lanes (DPP within a quad, no LDS); the group's first lane stores the record.  Full 16-byte-per-lane coalescing and
                         // 2 / 4 times the threads per picture.  0: the unit described above, max(16, b) columns, one record per thread.  Measured for 256 x 1080p pairs,
                         // the kernel alone at b = 32 / 64: 0 -> 435 / 930 us, 1 -> 310 / 310 us (profiles/r16_blockdiff.txt): 1 is kept
#endif
// log2 of a unit's columns at block size 1 << k, and a row's column groups: the width of a plane's grid of units (BD_LANE_GROUPS: a block row's groups are
// bw * (b / 16), also where the last block's right pieces lie outside the view, so that a group of lanes never straddles two blocks)
#if BD_LANE_GROUPS
#define BD_GROUP_LOG2(k) 4u
#define BD_ROW_GROUPS(w, k) ((k) > 4 ? (((uint32_t)(w) + (1u << (k)) - 1u) >> (k)) << ((k) - 4) : ((uint32_t)(w) + 15u) >> 4)
#else
#define BD_GROUP_LOG2(k) ((k) > 4 ? (uint32_t)(k) : 4u)
#define BD_ROW_GROUPS(w, k) (((uint32_t)(w) + (1u << BD_GROUP_LOG2(k)) - 1u) >> BD_GROUP_LOG2(k))
#endif
// units per thread at block size 1 << k: a unit is 2 * b * (its columns / 16) loads
#define BD_UNIT_LOADS(k) (2u << ((k) + BD_GROUP_LOG2(k) - 4u))
#define BD_UNITS(k) (BD_VECTORS / BD_UNIT_LOADS(k) ? BD_VECTORS / BD_UNIT_LOADS(k) : 1u)
#ifndef E264_EMU_BLOCKDIFF_STORE
#define E264_EMU_BLOCKDIFF_STORE(at) // what the host build counts (tests/emu/blockdiff_asan.cpp): record `at` of the pair's map stored
#endif

namespace {

typedef v4u E264_AS_GLOBAL __attribute__((aligned(1))) bd_gv4u; // 16 bytes at any address
typedef v2u E264_AS_GLOBAL __attribute__((aligned(8))) bd_grec; // one E264BlockDiff: the map is 16-byte aligned and a record 8 bytes

// 32-bit accumulators of a unit, index 0 for a vector's bytes 0 .. 7 and 1 for its bytes 8 .. 15.  A unit holds at most 64 x 64 = 4096 samples:
// s = sad <= 4096 * 255 < 2^21, m = sum a^2 + sum b^2 <= 2 * 4096 * 255^2 < 2^30, x = sum a b <= 4096 * 255^2 < 2^29, so 2 x < 2^30 and
// sse = m - 2 x <= 4096 * 255^2 < 2^32: nothing wraps, and the same bounds hold for the sums over a group of lanes (its units make up ONE block)
struct BdAcc { uint32_t s0, s1, m0, m1, x0, x1; };

#ifndef E264_HOST_INTRINSICS
E264_DEV uint32_t bd_sad4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }       // acc + the four |a_k - b_k| (v_sad_u8)
E264_DEV uint32_t bd_dot4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_udot4(a, b, acc, false); } // acc + the four a_k * b_k (v_dot4_u32_u8)
// x summed over the nv = 2 or 4 adjacent lanes of a group (every lane gets the sum): DPP quad permutes [1,0,3,2] and [2,3,0,1].  All lanes of the quad are active
// where this is called (they hold pieces of one block, so they leave the unit loop together).  `partner` is the host build's
template <class F> E264_DEV uint32_t bd_group_add(uint32_t x, const uint32_t nv, const uint32_t, F)
{
	x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xb1, 0xf, 0xf, false);
	if (nv == 4u) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4e, 0xf, 0xf, false);
	return x;
}
#else
E264_DEV uint32_t bd_sad4(uint32_t a, uint32_t b, uint32_t acc)
{
	for (int k = 0; k < 4; k++) { const uint32_t x = a >> (8 * k) & 255u, y = b >> (8 * k) & 255u; acc += x > y ? x - y : y - x; }
	return acc;
}
E264_DEV uint32_t bd_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
	for (int k = 0; k < 4; k++) acc += (a >> (8 * k) & 255u) * (b >> (8 * k) & 255u);
	return acc;
}
// the host's threads run one after the other: what the other lanes of the group hold is worked out here, partner(o, which) being member `which` of the sums of
// the lane whose number differs from this one's by xor o
template <class F> E264_DEV uint32_t bd_group_add(uint32_t x, const uint32_t nv, const uint32_t which, F partner)
{
	for (uint32_t o = 1; o < nv; o++) x += partner(o, which);
	return x;
}
#endif

E264_DEV void bd_store(gu8 *dst, const uint32_t at, const uint32_t sad, const uint32_t sse)
{
	*(bd_grec *)(dst + 8u * (uint64_t)at) = (v2u){sad, sse};
	E264_EMU_BLOCKDIFF_STORE(at);
}

// the 16 columns from column c < w of one row of both pictures, whose bytes lie at_a / at_b from the bases: a vector each where the columns all exist and both
// vectors end inside their slots, single bytes of the views otherwise
E264_DEV void bd_vector(BdAcc &r, const gu8 *base_a, const uint64_t at_a, const uint64_t slot_bytes_a, const gu8 *base_b, const uint64_t at_b, const uint64_t slot_bytes_b,
	const uint32_t c, const uint32_t w)
{
	if (c + 16u <= w && at_a + 16u <= slot_bytes_a && at_b + 16u <= slot_bytes_b) {
		const v4u a = *(const bd_gv4u *)(base_a + at_a), q = *(const bd_gv4u *)(base_b + at_b);
		const v4u x = a ^ q;
		if (x[0] | x[1] | x[2] | x[3]) {
			r.s0 = bd_sad4(a[0], q[0], r.s0); r.s0 = bd_sad4(a[1], q[1], r.s0);
			r.s1 = bd_sad4(a[2], q[2], r.s1); r.s1 = bd_sad4(a[3], q[3], r.s1);
			r.m0 = bd_dot4(a[0], a[0], r.m0); r.m0 = bd_dot4(q[0], q[0], r.m0); r.m0 = bd_dot4(a[1], a[1], r.m0); r.m0 = bd_dot4(q[1], q[1], r.m0);
			r.m1 = bd_dot4(a[2], a[2], r.m1); r.m1 = bd_dot4(q[2], q[2], r.m1); r.m1 = bd_dot4(a[3], a[3], r.m1); r.m1 = bd_dot4(q[3], q[3], r.m1);
			r.x0 = bd_dot4(a[0], q[0], r.x0); r.x0 = bd_dot4(a[1], q[1], r.x0);
			r.x1 = bd_dot4(a[2], q[2], r.x1); r.x1 = bd_dot4(a[3], q[3], r.x1);
		}
	} else {
		const uint32_t n = w - c < 16u ? w - c : 16u;
#pragma nounroll
		for (uint32_t i = 0; i < n; i++) {
			const uint32_t sa = base_a[at_a + i], sb = base_b[at_b + i], d = sa > sb ? sa - sb : sb - sa;
			if (i < 8u) { r.s0 += d; r.m0 += d * d; } // (d^2 straight into m: x stays)
			else { r.s1 += d; r.m1 += d * d; }
		}
	}
}

// a unit: `rows` rows of nv vectors from column c0 (at_a / at_b: the first row's bytes); columns from w on do not exist
E264_DEV BdAcc bd_unit(const gu8 *base_a, uint64_t at_a, const uint64_t stride_a, const uint64_t slot_bytes_a, const gu8 *base_b, uint64_t at_b, const uint64_t stride_b,
	const uint64_t slot_bytes_b, const uint32_t rows, const uint32_t nv, const uint32_t c0, const uint32_t w)
{
	BdAcc r = {0, 0, 0, 0, 0, 0};
#pragma nounroll
	for (uint32_t y = 0; y < rows; y++, at_a += stride_a, at_b += stride_b) {
#pragma nounroll
		for (uint32_t v = 0; v < nv && c0 + 16u * v < w; v++)
			bd_vector(r, base_a, at_a + 16u * v, slot_bytes_a, base_b, at_b + 16u * v, slot_bytes_b, c0 + 16u * v, w);
	}
	return r;
}

// thread `t` of `nt` (all the threads of this pair's workgroups, a multiple of 4): its units of the three planes.  Plane p of the two views has one size and k is
// 3 .. 6 (the host has checked); dst is the pair's map, 8-byte aligned
E264_DEV void blockdiff_thread(const E264View &view_a, const gu8 *base_a, const uint64_t slot_bytes_a, const E264View &view_b, const gu8 *base_b, const uint64_t slot_bytes_b,
	gu8 *dst, const uint32_t k, const uint32_t t, const uint32_t nt)
{
	const uint32_t b = 1u << k, gs = BD_GROUP_LOG2(k), nv = 1u << (gs - 4u); // block size; log2 of a unit's columns; its vectors per row
	const uint32_t gl = BD_LANE_GROUPS && k > 4u ? k - 4u : 0u, nl = 1u << gl;  // BD_LANE_GROUPS: log2 of the lanes that share a block, and their number
	uint32_t po = 0; // the plane's first record in the map
#pragma unroll
	for (int p = 0; p < 3; p++) {
		const uint32_t w = view_a.plane[p].width, h = view_a.plane[p].height;
		const uint64_t off_a = view_a.plane[p].offset, stride_a = view_a.plane[p].stride, off_b = view_b.plane[p].offset, stride_b = view_b.plane[p].stride;
		const uint32_t bw = (w + b - 1u) >> k, bh = (h + b - 1u) >> k;
		// the plane's units: bh block rows of ng column groups, unit u = Y * ng + g; this thread takes u = t, t + nt, ...
		const uint32_t ng = BD_ROW_GROUPS(w, k), dY = nt / ng, dg = nt - dY * ng;
		uint32_t Y = t / ng, g = t - Y * ng;
		while (Y < bh) {
			const uint32_t y0 = Y << k, rows = h - y0 < b ? h - y0 : b; // (b Y < h: Y < bh)
			const uint64_t row_a = off_a + (uint64_t)y0 * stride_a, row_b = off_b + (uint64_t)y0 * stride_b; // the block row's first bytes, from the bases
			// (G g < w: g < ng -- but for the pieces of BD_LANE_GROUPS that lie right of the view, which read nothing)
			const BdAcc r = bd_unit(base_a, row_a + (g << gs), stride_a, slot_bytes_a, base_b, row_b + (g << gs), stride_b, slot_bytes_b, rows, nv, g << gs, w);
			if (k == 3u) { // two records: the unit's columns 0 .. 7 and, where the view has them, 8 .. 15
				bd_store(dst, po + Y * bw + 2u * g, r.s0, r.m0 - 2u * r.x0);
				if (2u * g + 1u < bw)
					bd_store(dst, po + Y * bw + 2u * g + 1u, r.s1, r.m1 - 2u * r.x1);
			} else if (nl == 1u)
				bd_store(dst, po + Y * bw + g, r.s0 + r.s1, r.m0 + r.m1 - 2u * (r.x0 + r.x1));
			else { // the nl lanes t & ~(nl - 1) .. hold the pieces g & ~(nl - 1) .. of block g >> gl (nt and ng are multiples of nl): they are all here
				auto partner = [&](const uint32_t o, const uint32_t which) {
					const uint32_t go = g ^ o;
					const BdAcc q = bd_unit(base_a, row_a + (go << gs), stride_a, slot_bytes_a, base_b, row_b + (go << gs), stride_b, slot_bytes_b, rows, nv, go << gs, w);
					return which == 0u ? q.s0 + q.s1 : which == 1u ? q.m0 + q.m1 : q.x0 + q.x1;
				};
				const uint32_t s = bd_group_add(r.s0 + r.s1, nl, 0u, partner), m = bd_group_add(r.m0 + r.m1, nl, 1u, partner), x = bd_group_add(r.x0 + r.x1, nl, 2u, partner);
				if (!(g & (nl - 1u)))
					bd_store(dst, po + Y * bw + (g >> gl), s, m - 2u * x);
			}
			Y += dY; g += dg;
			if (g >= ng) { g -= ng; Y++; }
		}
		po += bw * bh;
	}
}

} // namespace
#endif
