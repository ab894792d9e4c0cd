// tests/emu/preview_asan.cpp -- TEST INFRASTRUCTURE: the preview kernel's body (edge264_amd/csrc/e264_preview.h, the source the device runs) compiled for the
// host and run over the threads of a grid, against include/edge264_preview.h's e264_preview_plane, with every plane in a heap block that ENDS with the
// plane's last byte and the preview in a heap block of EXACTLY its size.  Built with -fsanitize=address,undefined by tests/test_preview.py (into its temporary
// directory) and run as a child process: a load past the slot's end or a store outside the preview is reported by the sanitizer, a misaligned access that the
// source does not declare as such by the undefined-behaviour sanitizer, a wrong sum or clamp by the comparison.
//
// A case: width x height, stride = width + pad, the first byte a bytes into a 16-byte vector (a = 0..15), reduction k, threads of the grid.  The slot is a block of
// exactly a + (height - 1) * stride + width bytes; all three planes of the view are that plane, so the preview is three times the plane's, in a block of
// 3 * ow * oh bytes pre-filled with 0xa5 / 0x5a alternately.  Every byte of the slot is random, the padding too.  The body reports each store
// (E264_EMU_PREVIEW_STORE): every byte of the preview must have been stored exactly once, by whichever thread.
//   preview_asan            runs every case, prints a summary; exit status 0 when every preview was right
#include <vector>
static std::vector<unsigned> g_stores; // per byte of the preview: the stores that covered it
#define E264_EMU_PREVIEW_STORE(first_, n_) do { for (uint32_t i_ = 0; i_ < (n_); i_++) g_stores.at((first_) + i_)++; } while (0)
#include "emu_shims.h"
#include "../../edge264_amd/csrc/e264_preview.h"
#include "../../include/edge264_preview.h"

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

int main()
{
	static const int widths[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 65, 129, 1920}, heights[] = {1, 2, 3, 7, 9}, pads[] = {0, 1, 3, 16}, grids[] = {1, 64, 256, 768};
	unsigned long cases = 0, bad = 0;
	for (int w : widths) for (int h : heights) for (int pad : pads) for (int a = 0; a < 16; a++) {
		const size_t stride = (size_t)w + pad, bytes = a + (size_t)(h - 1) * stride + w;
		uint8_t *slot = (uint8_t *)malloc(bytes); // exactly the slot: what follows it is not the program's
		if (!slot || ((uintptr_t)slot & 15)) { fprintf(stderr, "malloc: %p\n", (void *)slot); return 2; }
		for (size_t i = 0; i < bytes; i++) slot[i] = (uint8_t)(rnd() >> 11);
		E264View view;
		for (int p = 0; p < 3; p++) view.plane[p] = (E264PlaneView){(uint32_t)a, (uint32_t)stride, (uint16_t)w, (uint16_t)h};
		for (int k = 1; k <= 3; k++) {
			unsigned ow, oh;
			if (!e264_preview_dims(w, h, k, &ow, &oh)) return 2;
			const size_t plane = (size_t)ow * oh, total = 3 * plane;
			std::vector<uint8_t> want(plane);
			e264_preview_plane(slot + a, stride, w, h, k, want.data(), ow);
			for (int nt : grids) {
				uint8_t *dst = (uint8_t *)malloc(total); // exactly the preview
				if (!dst) return 2;
				for (size_t i = 0; i < total; i++) dst[i] = i & 1 ? 0x5a : 0xa5;
				g_stores.assign(total, 0);
				for (int t = 0; t < nt; t++)
					preview_thread(view, slot, bytes, dst, (uint32_t)k, (uint32_t)t, (uint32_t)nt);
				cases++;
				bool ok = true;
				for (size_t i = 0; i < total && ok; i++)
					if (dst[i] != want[i % plane] || g_stores[i] != 1) {
						ok = false;
						if (bad < 20) fprintf(stderr, "w %d h %d stride %zu align %d k %d threads %d byte %zu of %zu: %u stored %u times, expected %u once\n", w, h, stride, a, k, nt,
							i, total, dst[i], g_stores[i], want[i % plane]);
					}
				bad += !ok;
				free(dst);
			}
		}
		free(slot);
	}
	printf("preview_asan: %lu cases, %lu wrong\n", cases, bad);
	return bad ? 1 : 0;
}
