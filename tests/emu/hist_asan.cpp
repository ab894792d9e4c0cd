// tests/emu/hist_asan.cpp -- TEST INFRASTRUCTURE: the histogram kernel's body (edge264_amd/csrc/e264_hist.h, the source the device runs; its add primitive is a
// plain add here) compiled for the host and run over the threads of a grid, every simulated workgroup of HS_NT threads adding into bins of its own and the
// workgroups' bins summed here as e264_hist.hip's flush sums them, against include/edge264_hist.h's e264_hist_plane.  The picture's plane lies in a heap block
// that ENDS with the plane's last byte (and begins with its first where the alignment asked for is 0); every workgroup's bins lie in a heap block of exactly
// 3 x 256 words.  Built with -fsanitize=address,undefined by tests/test_hist.py (into its temporary directory) and run as a child process: a load outside the
// plane's block or an add outside a bins block is reported by the address sanitizer, a misaligned access that the source does not declare as such by the
// undefined-behaviour sanitizer, a wrong record by the comparison.
//
// A case: width x height; stride = width + pad; the first byte `al` bytes into a 16-byte vector (0..15); a kind of content; threads of the grid (two of 1, 64,
// 256, 768 per content, in rotation).  The slot is a block of exactly al + (height - 1) * stride + width bytes, the padding random; all three planes of the view
// are that plane, so the three planes' bins must be equal.  Contents: 0 flat (one value), 1 flat per unit (one value per 16-column group and row), 2..17 fifteen
// equal bytes and one different at position 0..15 of every unit, 18 a ramp (x + y), 19 random, 20 only 0 and 255.
//   hist_asan            runs every case, prints a summary; exit status 0 when every record was right
#include <vector>
#include "emu_shims.h"
#include "../../edge264_amd/csrc/e264_hist.h"
#include "../../include/edge264_hist.h"

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// the bins of a grid of nt threads in workgroups of HS_NT, summed; false where the planes' bins do not sum to the workgroups'
static bool run_grid(const E264View &v, const uint8_t *s, size_t bytes, uint32_t nt, uint32_t got[HS_BINS])
{
	memset(got, 0, HS_BINS * sizeof(uint32_t));
	for (uint32_t t0 = 0; t0 < nt; t0 += HS_NT) {
		uint32_t *bins = (uint32_t *)calloc(HS_BINS, sizeof(uint32_t)); // exactly one copy of [3][256]
		if (!bins) return false;
		for (uint32_t t = t0; t < nt && t < t0 + HS_NT; t++)
			hist_thread(v, s, bytes, t, nt, bins);
		for (int i = 0; i < HS_BINS; i++) got[i] += bins[i];
		free(bins);
	}
	return true;
}

int main()
{
	static const int widths[] = {1, 15, 16, 17, 33, 130}, heights[] = {1, 4}, pads[] = {0, 1, 3, 16}, grids[] = {1, 64, 256, 768};
	unsigned long cases = 0, bad = 0, rot = 0;
	for (int w : widths) for (int h : heights) for (int pad : pads) for (int al = 0; al < 16; al++) {
		const size_t stride = (size_t)w + pad, bytes = al + (size_t)(h - 1) * stride + w;
		uint8_t *s = (uint8_t *)malloc(bytes); // exactly the slot: what follows it is not the program's
		if (!s || ((uintptr_t)s & 15)) { fprintf(stderr, "malloc: %p\n", (void *)s); return 2; }
		E264View v;
		for (int p = 0; p < 3; p++) v.plane[p] = (E264PlaneView){(uint32_t)al, (uint32_t)stride, (uint16_t)w, (uint16_t)h};
		for (int kind = 0; kind < 21; kind++) {
			for (size_t i = 0; i < bytes; i++) s[i] = (uint8_t)(rnd() >> 11);
			const uint8_t one = (uint8_t)(rnd() >> 9);
			for (int y = 0; y < h; y++)
				for (int x = 0; x < w; x++) {
					uint8_t &b = s[al + y * stride + x];
					const uint8_t unit = (uint8_t)(one + 37 * (x >> 4) + 101 * y);
					if (kind == 0) b = one;
					else if (kind == 1) b = unit;
					else if (kind < 18) b = (x & 15) == kind - 2 ? (uint8_t)(unit + 1 + (x >> 4)) : unit;
					else if (kind == 18) b = (uint8_t)(x + y + one);
					else if (kind == 20) b = (b & 1) ? 255 : 0;
				}
			uint32_t want[256];
			e264_hist_plane(s + al, stride, w, h, want);
			for (int g = 0; g < 2; g++) {
				const int nt = grids[(rot + kind + 2 * g) & 3];
				uint32_t got[HS_BINS];
				if (!run_grid(v, s, bytes, (uint32_t)nt, got)) return 2;
				cases++;
				bool ok = true;
				for (int p = 0; p < 3; p++) ok = ok && !memcmp(got + 256 * p, want, sizeof(want));
				if (!ok && bad < 20) {
					int at = 0;
					while (at < 255 && got[at] == want[at]) at++;
					fprintf(stderr, "w %d h %d stride %zu align %d kind %d threads %d: luma bin %d is %u, expected %u\n", w, h, stride, al, kind, nt, at, got[at], want[at]);
				}
				bad += !ok;
			}
		}
		rot++;
		free(s);
	}
	printf("hist_asan: %lu cases, %lu wrong\n", cases, bad);
	return bad ? 1 : 0;
}
