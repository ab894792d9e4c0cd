// tests/emu/blockstat_asan.cpp -- TEST INFRASTRUCTURE: the block statistics kernel's body (edge264_amd/csrc/e264_blockstat.h, the source the device runs) compiled
// for the host and run over the threads of a grid, against the plain definition written out below (and include/edge264_blockstat.h's e264_blockstat_plane), with
// the plane in a heap block that BEGINS with the view's first byte and ENDS with its last byte (the first byte `al` bytes into a 16-byte vector: the block is
// handed out at a 16-byte boundary and the view starts al bytes into it, those al bytes being the only ones of the block that are not between the view's first
// and last) and the map in a heap block of EXACTLY its size.  Built with -fsanitize=address,undefined by tests/test_blockstat.py (into its temporary directory)
// and run as a child process: a load outside the picture's block or a store outside the map is reported by the address sanitizer, a misaligned access that the
// source does not declare as such by the undefined-behaviour sanitizer, a wrong sum -- a pair taken from the padding, a sixteenth pair not masked off, a row
// below the view -- by the comparison, since every byte of the block is random, the padding too.
//
// A case: width x height, both from tests/test_blockdiff.py's SIZES, squared off against each other; stride = width + pad, pad in {0, 1, 3, 16}; al = 0 .. 15;
// block size 1 << k for every k = 3 .. 6; the grid has 1, 64, 256 or 768 threads (in rotation over the cases).  al == 0: the slot is exactly the view, first byte
// to last.  All three planes of a view are that plane, so the map is three times the plane's, in a block of 3 * bw * bh records pre-filled with 0xa5.  The body
// reports each store (E264_EMU_BLOCKSTAT_STORE): every record of the map must have been stored exactly once, by whichever thread.
//   The last cases: one 64 x 64 block of 255 (the largest sum and sumsq a record can hold) and one 64 x 64 checkerboard of 0 and 255 (the largest gh and gv) at
//   every k.
//   blockstat_asan            runs every case, prints a summary; exit status 0 when every map was right
#include <vector>
static std::vector<unsigned> g_stores; // per record of the map: the stores that covered it
#define E264_EMU_BLOCKSTAT_STORE(at_) (g_stores.at(at_)++)
#include "emu_shims.h"
#include "../../edge264_amd/csrc/e264_blockstat.h"
#include "../../include/edge264_blockstat.h"

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// the plain definition: every sample adds itself and its square to its block, every pair inside the plane its difference to the block of its left / top sample
static std::vector<E264BlockStat> plain(const uint8_t *s, size_t stride, int w, int h, int k)
{
	const int b = 1 << k, bw = (w + b - 1) / b, bh = (h + b - 1) / b;
	std::vector<E264BlockStat> out((size_t)bw * bh, (E264BlockStat){0, 0, 0, 0});
	for (int y = 0; y < h; y++)
		for (int x = 0; x < w; x++) {
			E264BlockStat &r = out[(size_t)(y / b) * bw + x / b];
			const int v = s[y * stride + x];
			r.sum += (uint32_t)v;
			r.sumsq += (uint32_t)(v * v);
			if (x + 1 < w) r.gh += (uint32_t)abs(s[y * stride + x + 1] - v);
			if (y + 1 < h) r.gv += (uint32_t)abs(s[(y + 1) * stride + x] - v);
		}
	return out;
}

// one grid over one picture: true when the three planes' maps equal `want` and every record was stored once
static bool run_case(const E264View &v, const uint8_t *slot, size_t bytes, int k, int nt, const std::vector<E264BlockStat> &want, const char *what)
{
	const size_t plane = want.size(), total = 3 * plane;
	E264BlockStat *map = (E264BlockStat *)malloc(total * sizeof(E264BlockStat)); // exactly the map
	if (!map) abort();
	memset(map, 0xa5, total * sizeof(E264BlockStat));
	g_stores.assign(total, 0);
	for (int t = 0; t < nt; t++)
		blockstat_thread(v, slot, bytes, (uint8_t *)map, (uint32_t)k, (uint32_t)t, (uint32_t)nt);
	bool ok = true;
	for (size_t i = 0; i < total && ok; i++) {
		const E264BlockStat &m = map[i], &e = want[i % plane];
		if (m.sum != e.sum || m.sumsq != e.sumsq || m.gh != e.gh || m.gv != e.gv || g_stores[i] != 1) {
			ok = false;
			if (*what) fprintf(stderr, "%s k %d threads %d record %zu of %zu: %u %u %u %u stored %u times, expected %u %u %u %u once\n", what, k, nt, i, total, m.sum, m.sumsq,
				m.gh, m.gv, g_stores[i], e.sum, e.sumsq, e.gh, e.gv);
		}
	}
	free(map);
	return ok;
}

int main()
{
	static const int sizes[] = {1, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 129}, pads[] = {0, 1, 3, 16}, grids[] = {1, 64, 256, 768};
	unsigned long cases = 0, bad = 0, rot = 0;
	char what[160];
	for (int w : sizes) for (int h : sizes) for (int pad : pads) for (int al = 0; al < 16; al++) {
		const size_t stride = (size_t)w + pad, bytes = al + (size_t)(h - 1) * stride + w;
		uint8_t *slot = (uint8_t *)malloc(bytes); // exactly the slot: what follows it is not the program's
		if (!slot || ((uintptr_t)slot & 15)) { fprintf(stderr, "malloc: %p\n", (void *)slot); return 2; }
		for (size_t i = 0; i < bytes; i++) slot[i] = (uint8_t)(rnd() >> 11);
		E264View v;
		for (int p = 0; p < 3; p++) v.plane[p] = (E264PlaneView){(uint32_t)al, (uint32_t)stride, (uint16_t)w, (uint16_t)h};
		for (int k = 3; k <= 6; k++) {
			unsigned bw, bh;
			if (!e264_blockstat_dims(w, h, k, &bw, &bh)) return 2;
			const std::vector<E264BlockStat> want = plain(slot + al, stride, w, h, k);
			std::vector<E264BlockStat> hdr((size_t)bw * bh);
			e264_blockstat_plane(slot + al, stride, w, h, k, hdr.data());
			if (want.size() != hdr.size() || memcmp(want.data(), hdr.data(), want.size() * sizeof(E264BlockStat))) { fprintf(stderr, "the header differs from the plain definition: w %d h %d k %d\n", w, h, k); bad++; }
			const int nt = grids[(rot + k) & 3];
			snprintf(what, sizeof what, "w %d h %d stride %zu align %d", w, h, stride, al);
			cases++;
			bad += !run_case(v, slot, bytes, k, nt, want, bad < 20 ? what : "");
		}
		rot++;
		free(slot);
	}
	for (int pattern = 0; pattern < 2; pattern++) // 64 x 64 samples of 255, then a checkerboard of 0 and 255: one thread and many
		for (int k = 3; k <= 6; k++) {
			const size_t n = 64 * 64;
			uint8_t *s = (uint8_t *)malloc(n);
			if (!s) return 2;
			for (size_t i = 0; i < n; i++) s[i] = pattern ? (uint8_t)(((i >> 6) + i) & 1 ? 255 : 0) : 255;
			E264View v;
			for (int p = 0; p < 3; p++) v.plane[p] = (E264PlaneView){0, 64, 64, 64};
			const std::vector<E264BlockStat> want = plain(s, 64, 64, 64, k);
			if (k == 6 && (pattern ? want[0].gh != 64u * 63u * 255u || want[0].gv != 64u * 63u * 255u : want[0].sum != 4096u * 255u || want[0].sumsq != 4096u * 65025u)) bad++;
			for (int nt : {1, 256}) {
				cases++;
				bad += !run_case(v, s, n, k, nt, want, pattern ? "64 x 64 checkerboard" : "64 x 64 of 255");
			}
			free(s);
		}
	printf("blockstat_asan: %lu cases, %lu wrong\n", cases, bad);
	return bad ? 1 : 0;
}
