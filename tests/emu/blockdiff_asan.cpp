// tests/emu/blockdiff_asan.cpp -- TEST INFRASTRUCTURE: the block difference kernel's body (edge264_amd/csrc/e264_blockdiff.h, the source the device runs) compiled
// for the host and run over the threads of a grid, against include/edge264_blockdiff.h's e264_blockdiff_plane, with each picture's plane in a heap block of its
// own that ENDS with the plane's last byte (and begins with its first where the alignment asked for is 0) and the map in a heap block of EXACTLY its size.  Built
// with -fsanitize=address,undefined by tests/test_blockdiff.py (into its temporary directory) and run as a child process: a load outside either picture's block or
// a store outside the map is reported by the address sanitizer, a misaligned access that the source does not declare as such by the undefined-behaviour
// sanitizer, a wrong sum by the comparison.
//
// A case: width x height; per side a stride = width + pad and the first byte `al` bytes into a 16-byte vector (A: 0..15, B: 0, 1, 7, 15), so the two pictures'
// rows differ in alignment; block size 1 << k for every k = 3 .. 6; B's samples are A's with 0, 1, 2 or many changed and the grid has 1, 64, 256 or 768 threads
// (both in rotation over the cases).  A side's slot is a block of exactly al + (height - 1) * stride + width bytes, every byte random, the padding too (each side
// its own); all three planes of a view are that plane, so the map is three times the plane's, in a block of 3 * bw * bh records pre-filled with 0xa5.  The body
// reports each store (E264_EMU_BLOCKDIFF_STORE): every record of the map must have been stored exactly once, by whichever thread.
//   The last cases: one 64 x 64 block of 0 against 255 at every k -- at k = 6 the largest sad and sse a record can hold.
//   blockdiff_asan            runs every case, prints a summary; exit status 0 when every map was right
#include <vector>
static std::vector<unsigned> g_stores; // per record of the map: the stores that covered it
#define E264_EMU_BLOCKDIFF_STORE(at_) (g_stores.at(at_)++)
#include "emu_shims.h"
#include "../../edge264_amd/csrc/e264_blockdiff.h"
#include "../../include/edge264_blockdiff.h"

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// one grid over one pair: true when the three planes' maps equal `want` and every record was stored once
static bool run_case(const E264View &va, const uint8_t *sa, size_t bytes_a, const E264View &vb, const uint8_t *sb, size_t bytes_b, int k, int nt,
	const std::vector<E264BlockDiff> &want, const char *what)
{
	const size_t plane = want.size(), total = 3 * plane;
	E264BlockDiff *map = (E264BlockDiff *)malloc(total * sizeof(E264BlockDiff)); // exactly the map
	if (!map) abort();
	memset(map, 0xa5, total * sizeof(E264BlockDiff));
	g_stores.assign(total, 0);
	for (int t = 0; t < nt; t++)
		blockdiff_thread(va, sa, bytes_a, vb, sb, bytes_b, (uint8_t *)map, (uint32_t)k, (uint32_t)t, (uint32_t)nt);
	bool ok = true;
	for (size_t i = 0; i < total && ok; i++)
		if (map[i].sad != want[i % plane].sad || map[i].sse != want[i % plane].sse || g_stores[i] != 1) {
			ok = false;
			if (*what) fprintf(stderr, "%s k %d threads %d record %zu of %zu: sad %u sse %u stored %u times, expected %u %u once\n", what, k, nt, i, total, map[i].sad, map[i].sse,
				g_stores[i], want[i % plane].sad, want[i % plane].sse);
		}
	free(map);
	return ok;
}

int main()
{
	static const int widths[] = {1, 15, 16, 17, 33, 130}, heights[] = {1, 9, 70}, pads[] = {0, 1, 3, 16}, aligns_b[] = {0, 1, 7, 15}, grids[] = {1, 64, 256, 768};
	unsigned long cases = 0, bad = 0, rot = 0;
	char what[160];
	for (int w : widths) for (int h : heights) for (int pad_a : pads) for (int pad_b : pads) for (int al_a = 0; al_a < 16; al_a++) for (int al_b : aligns_b) {
		const size_t stride_a = (size_t)w + pad_a, stride_b = (size_t)w + pad_b;
		const size_t bytes_a = al_a + (size_t)(h - 1) * stride_a + w, bytes_b = al_b + (size_t)(h - 1) * stride_b + w;
		uint8_t *sa = (uint8_t *)malloc(bytes_a), *sb = (uint8_t *)malloc(bytes_b); // exactly the slots: what follows them is not the program's
		if (!sa || !sb || (((uintptr_t)sa | (uintptr_t)sb) & 15)) { fprintf(stderr, "malloc: %p %p\n", (void *)sa, (void *)sb); return 2; }
		for (size_t i = 0; i < bytes_a; i++) sa[i] = (uint8_t)(rnd() >> 11);
		E264View va, vb;
		for (int p = 0; p < 3; p++) {
			va.plane[p] = (E264PlaneView){(uint32_t)al_a, (uint32_t)stride_a, (uint16_t)w, (uint16_t)h};
			vb.plane[p] = (E264PlaneView){(uint32_t)al_b, (uint32_t)stride_b, (uint16_t)w, (uint16_t)h};
		}
		for (int k = 3; k <= 6; k++) {
			const int change = (int)((rot + k) & 3); // B = A with 0, 1, 2 or many samples changed
			for (size_t i = 0; i < bytes_b; i++) sb[i] = (uint8_t)(rnd() >> 11);
			for (int y = 0; y < h; y++) memcpy(sb + al_b + y * stride_b, sa + al_a + y * stride_a, w);
			const int n = change < 3 ? change : 3 + (int)(rnd() % (uint32_t)(w * h));
			for (int c = 0; c < n; c++) {
				const uint32_t i = rnd() % (uint32_t)(w * h);
				sb[al_b + (i / w) * stride_b + i % w] ^= (uint8_t)(1u + rnd() % 255u);
			}
			unsigned bw, bh;
			if (!e264_blockdiff_dims(w, h, k, &bw, &bh)) return 2;
			std::vector<E264BlockDiff> want((size_t)bw * bh);
			e264_blockdiff_plane(sa + al_a, stride_a, sb + al_b, stride_b, w, h, k, want.data());
			const int nt = grids[(rot / 4 + k) & 3];
			snprintf(what, sizeof what, "w %d h %d strides %zu %zu aligns %d %d changes %d", w, h, stride_a, stride_b, al_a, al_b, n);
			cases++;
			const bool ok = run_case(va, sa, bytes_a, vb, sb, bytes_b, k, nt, want, bad < 20 ? what : "");
			bad += !ok;
		}
		rot++;
		free(sa); free(sb);
	}
	for (int k = 3; k <= 6; k++) { // 64 x 64 samples of 0 against 255, one thread and many
		const size_t n = 64 * 64;
		uint8_t *sa = (uint8_t *)malloc(n), *sb = (uint8_t *)malloc(n);
		if (!sa || !sb) return 2;
		memset(sa, 0, n); memset(sb, 255, n);
		E264View v;
		for (int p = 0; p < 3; p++) v.plane[p] = (E264PlaneView){0, 64, 64, 64};
		const uint32_t b = 1u << k, per = 64u >> k;
		const std::vector<E264BlockDiff> want((size_t)per * per, (E264BlockDiff){b * b * 255u, b * b * 65025u});
		for (int nt : {1, 256}) {
			cases++;
			bad += !run_case(v, sa, n, v, sb, n, k, nt, want, "64 x 64, 0 against 255");
		}
		free(sa); free(sb);
	}
	printf("blockdiff_asan: %lu cases, %lu wrong\n", cases, bad);
	return bad ? 1 : 0;
}
