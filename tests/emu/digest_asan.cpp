// tests/emu/digest_asan.cpp -- TEST INFRASTRUCTURE: the digest kernel's body (edge264_amd/csrc/e264_digest.h, the source the device runs) compiled for the
// host and summed over the threads of a grid, against include/edge264_digest.h's e264_digest_plane, with every plane in a heap block that ENDS with the
// plane's last byte.  Built with -fsanitize=address,undefined by tests/test_digest.py (into its temporary directory) and run as a child process: a load past
// the slot's end -- the aligned 16-byte vector that holds a row's tail -- is reported by the sanitizer, a wrong mask or index by the comparison.
//
// A case: width x height, stride = width + pad, the first byte a bytes into a 16-byte vector (a = 0..15).  The slot is a block of EXACTLY
// a + (height - 1) * stride + width bytes (malloc: 16-byte aligned, like a device allocation), the plane starts a bytes in and ends with the block; for a = 0 its
// first byte is the block's first as well.  (The a bytes in front belong to the slot: the kernel may read an aligned vector's padding inside the slot, and the
// sanitizer could not tell bytes of one 8-byte granule apart on that side anyway.)  All three planes of the view are that plane.  Every byte of the block is
// random, the padding too.
//   digest_asan            runs every case, prints a summary; exit status 0 when every sum was right
#include "emu_shims.h"
#include "../../edge264_amd/csrc/e264_digest.h"
#include "../../include/edge264_digest.h"

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

int main()
{
	static const int widths[] = {1, 2, 3, 4, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 255, 257, 1920}, heights[] = {1, 2, 3, 9}, pads[] = {0, 1, 3, 16},
		grids[] = {1, 64, 256, 768, 1792};
	unsigned long cases = 0, bad = 0;
	for (int w : widths) for (int h : heights) for (int pad : pads) for (int a = 0; a < 16; a++) {
		const size_t stride = (size_t)w + pad, bytes = a + (size_t)(h - 1) * stride + w;
		uint8_t *slot = (uint8_t *)malloc(bytes); // exactly the slot: what follows it is not the program's
		if (!slot || ((uintptr_t)slot & 15)) { fprintf(stderr, "malloc: %p\n", (void *)slot); return 2; }
		for (size_t i = 0; i < bytes; i++) slot[i] = (uint8_t)(rnd() >> 11);
		const uint64_t want = e264_digest_plane(slot + a, stride, w, h);
		E264View view;
		for (int p = 0; p < 3; p++) view.plane[p] = (E264PlaneView){(uint32_t)a, (uint32_t)stride, (uint16_t)w, (uint16_t)h};
		for (int nt : grids) {
			DigestSums sum = {{0, 0, 0}};
			for (int t = 0; t < nt; t++) {
				const DigestSums s = digest_thread(view, slot, bytes, (uint32_t)t, (uint32_t)nt);
				for (int p = 0; p < 3; p++) sum.d[p] += s.d[p];
			}
			cases++;
			for (int p = 0; p < 3; p++)
				if (sum.d[p] != want) {
					if (bad++ < 20) fprintf(stderr, "w %d h %d stride %zu align %d threads %d plane %d: %016llx, expected %016llx\n", w, h, stride, a, nt, p,
						(unsigned long long)sum.d[p], (unsigned long long)want);
					break;
				}
		}
		free(slot);
	}
	printf("digest_asan: %lu cases, %lu wrong\n", cases, bad);
	return bad ? 1 : 0;
}
