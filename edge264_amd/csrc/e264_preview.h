// e264_preview.h -- e264_preview_kernel's body: the reduced preview of include/edge264_hip.h (version 1) of one picture, read where it lies in its slot (E264View).
// For a plane of w x h samples and f = 1 << k (k = 1, 2, 3):  P[Y][X] = (sum of the f x f box at (f X, f Y), columns and rows clamped to the plane, + f * f / 2) >> 2 k,
// ow = ceil(w / f) by oh = ceil(h / f) bytes, written tight; the three planes follow each other (Y | Cb | Cr).
// A thread's unit of work is (plane, output row Y, column group j): the 16 input columns 16 j .. 16 j + 15 of the f input rows of Y, which give 16 / f = 8, 4 or 2
// output bytes.  Thread t of nt takes units t, t + nt, ... (Y and j kept up without a division per unit, as digest_thread does).
//   An INTERIOR unit -- its 16 columns and its f rows all exist -- loads one 16-byte vector per row at the row's own address, whatever its alignment (global memory
//   takes unaligned vector accesses on gfx9+; the vector types here are 1-byte aligned, so the host build's loads are defined as well), sums in registers and
//   stores its 8, 4 or 2 bytes with one store.  Every such vector lies inside a row of the view, so inside the slot for a view e264hip_view_check has accepted;
//   the body compares the last vector's end with slot_bytes all the same and reads a unit it fails for byte by byte, like the digest.
//   Every OTHER unit -- the last columns of a row, rows clamped at the bottom -- reads single bytes at clamped coordinates: bytes of the view only.
// So no byte outside [base, base + slot_bytes) is read, and since the units partition each plane's output (unit j of row Y writes columns (16 / f) j up to
// min(ow, (16 / f) (j + 1)), at least one) every byte of the preview is written exactly once, without atomics, and none outside it
// (tests/emu/preview_asan.cpp holds this source to both, compiled for the host under the address sanitizer).
// Cost, counted in the assembly, addresses and loop included: about 63 VALU instructions per interior unit at f = 8 (128 samples: 0.5 per sample), 47 at f = 4
// (64 samples: 0.7), 68 at f = 2 (32 samples: 2.1) against the digest's ~11 per sample, so the pass is bound by its reads (profiles/r13_preview.txt).
#ifndef E264_PREVIEW_H
#define E264_PREVIEW_H
#include "e264_dev.h"

#define PV_NT 256     // threads of a workgroup
#ifndef PV_VECTORS
#define PV_VECTORS 64 // 16-byte loads per thread a picture's chunk count aims at (e264_preview_chunks): 8, 16 or 32 units, which share the thread's set-up -- two
                      // divisions per plane.  Measured for 256 x 1080p at k = 1 / 2 / 3: 8 loads 185 / 164 / 269 us, 16: 197 / 163 / 200, 32: 199 / 170 / 178, 64: 189 / 157 / 162
                      // (`make variant DEFS=-DPV_VECTORS=..`, profiles/r13_preview.txt)
#endif
#define PV_ROW_GROUPS(w) (((uint32_t)(w) + 15u) >> 4) // column groups of a row of w samples: the width of a plane's grid of units
#ifndef E264_EMU_PREVIEW_STORE
#define E264_EMU_PREVIEW_STORE(at, n) // what the host build counts (tests/emu/preview_asan.cpp): n bytes stored `at` bytes into the picture's preview
#endif

namespace {

typedef v4u E264_AS_GLOBAL __attribute__((aligned(1))) pv_gv4u; // 16 bytes at any address
typedef v2u E264_AS_GLOBAL __attribute__((aligned(1))) pv_gv2u;
typedef uint32_t E264_AS_GLOBAL __attribute__((aligned(1))) pv_gu32;
typedef uint16_t E264_AS_GLOBAL __attribute__((aligned(1))) pv_gu16;

// acc + the four bytes of d (v_sad_u8 against 0)
#ifndef E264_HOST_INTRINSICS
E264_DEV uint32_t pv_sum4(uint32_t d, uint32_t acc) { return __builtin_amdgcn_sad_u8(d, 0u, acc); }
#else
E264_DEV uint32_t pv_sum4(uint32_t d, uint32_t acc) { return acc + (d & 255u) + (d >> 8 & 255u) + (d >> 16 & 255u) + (d >> 24); }
#endif

// an interior unit: F rows of 16 bytes at src, `stride` apart, to 16 / F bytes at dst
template <int K> E264_DEV void preview_interior(const gu8 *src, const uint64_t stride, gu8 *dst)
{
	constexpr int F = 1 << K;
	v4u q[F];
#pragma unroll
	for (int dy = 0; dy < F; dy++) // (all the loads first: F of them in flight)
		q[dy] = *(const pv_gv4u *)(src + dy * stride);
	if (K == 1) {
		uint32_t o[4];
#pragma unroll
		for (int c = 0; c < 4; c++) { // two pair sums per dword in packed 16-bit (<= 510 each), the two rows and the rounding added: <= 1022, no carry between the halves
			const uint32_t s = (q[0][c] & 0x00ff00ffu) + (q[0][c] >> 8 & 0x00ff00ffu) + (q[1][c] & 0x00ff00ffu) + (q[1][c] >> 8 & 0x00ff00ffu) + 0x00020002u;
			const uint32_t b = s >> 2 & 0x00ff00ffu; // the two results, in bytes 0 and 2
			o[c] = (b | b >> 8) & 0xffffu;
		}
		*(pv_gv2u *)dst = (v2u){o[0] | o[1] << 16, o[2] | o[3] << 16};
	} else if (K == 2) {
		uint32_t a[4] = {8u, 8u, 8u, 8u}; // a dword of a row is one box's row
#pragma unroll
		for (int dy = 0; dy < F; dy++)
#pragma unroll
			for (int c = 0; c < 4; c++)
				a[c] = pv_sum4(q[dy][c], a[c]);
		*(pv_gu32 *)dst = a[0] >> 4 | a[1] >> 4 << 8 | a[2] >> 4 << 16 | a[3] >> 4 << 24;
	} else {
		uint32_t a[2] = {32u, 32u}; // two dwords of a row are one box's row
#pragma unroll
		for (int dy = 0; dy < F; dy++)
#pragma unroll
			for (int c = 0; c < 4; c++)
				a[c >> 1] = pv_sum4(q[dy][c], a[c >> 1]);
		*(pv_gu16 *)dst = (uint16_t)(a[0] >> 6 | a[1] >> 6 << 8);
	}
}

// any other unit: output columns X0 .. X1 - 1 of output row Y, every sample read as a single byte at clamped coordinates.  plane: the view's first sample
template <int K> E264_DEV void preview_edge(const gu8 *plane, const uint64_t stride, const uint32_t w, const uint32_t h, const uint32_t Y, const uint32_t X0, const uint32_t X1,
	gu8 *dst_row, const uint32_t at_row)
{
	constexpr uint32_t F = 1u << K;
#pragma nounroll
	for (uint32_t X = X0; X < X1; X++) { // (rolled loops: the few units of a plane's right and bottom edges are not worth the registers of an unrolled form)
		uint32_t sum = 1u << (2 * K - 1);
#pragma nounroll
		for (uint32_t dy = 0; dy < F; dy++) {
			const gu8 *row = plane + (uint64_t)min(F * Y + dy, h - 1u) * stride;
#pragma nounroll
			for (uint32_t dx = 0; dx < F; dx++)
				sum += row[min(F * X + dx, w - 1u)];
		}
		dst_row[X] = (uint8_t)(sum >> (2 * K));
		E264_EMU_PREVIEW_STORE(at_row + X, 1u);
	}
}

template <int K> E264_DEV void preview_planes(const E264View &view, const gu8 *base, const uint64_t slot_bytes, gu8 *dst, const uint32_t t, const uint32_t nt)
{
	constexpr uint32_t F = 1u << K, N = 16u >> K; // box size; output bytes of a unit
	uint32_t po = 0; // the plane's first byte in the preview
#pragma unroll
	for (int p = 0; p < 3; p++) {
		const uint32_t w = view.plane[p].width, h = view.plane[p].height;
		const uint64_t off = view.plane[p].offset, stride = view.plane[p].stride;
		const uint32_t ow = (w + F - 1u) >> K, oh = (h + F - 1u) >> K;
		// the plane's units: oh rows of nj column groups, unit u = Y * nj + j; this thread takes u = t, t + nt, ...
		const uint32_t nj = PV_ROW_GROUPS(w), dY = nt / nj, dj = nt - dY * nj;
		uint32_t Y = t / nj, j = t - Y * nj;
		while (Y < oh) {
			const uint64_t first = off + (uint64_t)(F * Y) * stride + 16u * j; // the unit's first byte, from base
			const uint32_t at = po + Y * ow + N * j;                             // ... and its first output byte, from dst
			if (16u * j + 16u <= w && F * Y + F <= h && first + (F - 1u) * stride + 16u <= slot_bytes) {
				preview_interior<K>(base + first, stride, dst + at); // (N <= ow - N j: 16 j + 16 <= w)
				E264_EMU_PREVIEW_STORE(at, N);
			} else
				preview_edge<K>(base + off, stride, w, h, Y, N * j, min(ow, N * j + N), dst + (po + Y * ow), po + Y * ow);
			Y += dY; j += dj;
			if (j >= nj) { j -= nj; Y++; }
		}
		po += ow * oh;
	}
}

// thread `t` of `nt` (all the threads of this picture's workgroups): its units of the three planes.  k = 1, 2 or 3 (the host has checked)
E264_DEV void preview_thread(const E264View &view, const gu8 *base, const uint64_t slot_bytes, gu8 *dst, const uint32_t k, const uint32_t t, const uint32_t nt)
{
	if (k == 1) preview_planes<1>(view, base, slot_bytes, dst, t, nt);
	else if (k == 2) preview_planes<2>(view, base, slot_bytes, dst, t, nt);
	else preview_planes<3>(view, base, slot_bytes, dst, t, nt);
}

} // namespace
#endif
