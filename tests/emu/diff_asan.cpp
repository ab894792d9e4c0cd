// tests/emu/diff_asan.cpp -- TEST INFRASTRUCTURE: the diff kernel's body (edge264_amd/csrc/e264_diff.h, the source the device runs) compiled for the host and run
// over the threads of a grid, the threads' partial records combined here as e264_diff.hip combines them (sums, max, min), against include/edge264_diff.h's
// e264_diff_plane, with each picture's plane in a heap block of its own that ENDS with the plane's last byte (and begins with its first where the alignment
// asked for is 0).  Built with -fsanitize=address,undefined by tests/test_diff.py (into its temporary directory) and run as a child process: a load outside
// either block is reported by the address sanitizer, a misaligned access that the source does not declare as such by the undefined-behaviour sanitizer, a wrong
// record by the comparison.
//
// A case: width x height; per side a stride = width + pad and the first byte `al` bytes into a 16-byte vector (A: 0..15, B: 0, 1, 7, 15), so the two pictures'
// rows differ in alignment; B's samples are A's with 0, 1, 2 or many changed; threads of the grid.  A side's slot is a block of exactly
// al + (height - 1) * stride + width bytes, every byte random, the padding too (each side its own); all three planes of a view are that plane, so the three
// records must be equal.
//   The last case runs ONE thread (nt = 1) over a 4096 x 4096 plane of 0 against 255: sad = 255 * 2^24, sse = 65025 * 2^24, count = 2^24 -- a 32-bit
//   accumulator that the body did not spill in time would show here.
//   diff_asan            runs every case, prints a summary; exit status 0 when every record was right
#include <vector>
#include "emu_shims.h"
#include "../../edge264_amd/csrc/e264_diff.h"
#include "../../include/edge264_diff.h"

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// the records of a grid of nt threads, combined
static void run_grid(const E264View &va, const uint8_t *sa, size_t bytes_a, const E264View &vb, const uint8_t *sb, size_t bytes_b, uint32_t nt, E264PlaneDiff got[3])
{
	for (int p = 0; p < 3; p++) got[p] = (E264PlaneDiff){0, 0, 0, E264_DIFF_NONE, 0, 0};
	for (uint32_t t = 0; t < nt; t++) {
		const DiffPart r = diff_thread(va, sa, bytes_a, vb, sb, bytes_b, t, nt);
		for (int p = 0; p < 3; p++) {
			got[p].sad += r.sad[p]; got[p].sse += r.sse[p]; got[p].count += r.count[p];
			if (r.first[p] < got[p].first) got[p].first = r.first[p];
			if (r.max[p] > got[p].max) got[p].max = r.max[p];
			if ((r.count[p] == 0) != (r.first[p] == E264_DIFF_NONE)) got[p].zero = 1; // (a part that names a first sample has counted one)
		}
	}
}
static bool same(const E264PlaneDiff &a, const E264PlaneDiff &b)
{
	return a.sad == b.sad && a.sse == b.sse && a.count == b.count && a.first == b.first && a.max == b.max && a.zero == b.zero;
}

int main()
{
	static const int widths[] = {1, 15, 16, 17, 33, 130}, heights[] = {1, 4}, pads[] = {0, 1, 3, 16}, aligns_b[] = {0, 1, 7, 15}, grids[] = {1, 64, 256, 768};
	unsigned long cases = 0, bad = 0, rot = 0;
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
		for (int change = 0; change < 4; change++) { // B = A with 0, 1, 2 or many samples changed
			for (size_t i = 0; i < bytes_b; i++) sb[i] = (uint8_t)(rnd() >> 11);
			for (int y = 0; y < h; y++) memcpy(sb + al_b + y * stride_b, sa + al_a + y * stride_a, w);
			const int n = change < 3 ? change : 3 + (int)(rnd() % (uint32_t)(w * h));
			for (int k = 0; k < n; k++) {
				const uint32_t i = rnd() % (uint32_t)(w * h);
				sb[al_b + (i / w) * stride_b + i % w] ^= (uint8_t)(1u + rnd() % 255u);
			}
			E264PlaneDiff want;
			e264_diff_plane(sa + al_a, stride_a, sb + al_b, stride_b, w, h, &want);
			for (int g = 0; g < 2; g++) {
				const int nt = grids[(rot + change + 2 * g) & 3];
				E264PlaneDiff got[3];
				run_grid(va, sa, bytes_a, vb, sb, bytes_b, (uint32_t)nt, got);
				cases++;
				bool ok = true;
				for (int p = 0; p < 3; p++) ok = ok && same(got[p], want);
				if (!ok && bad < 20)
					fprintf(stderr, "w %d h %d strides %zu %zu aligns %d %d changes %d threads %d: sad %llu sse %llu count %u first %u max %u flag %u, expected %llu %llu %u %u %u\n",
						w, h, stride_a, stride_b, al_a, al_b, n, nt, (unsigned long long)got[0].sad, (unsigned long long)got[0].sse, got[0].count, got[0].first, got[0].max,
						got[0].zero, (unsigned long long)want.sad, (unsigned long long)want.sse, want.count, want.first, want.max);
				bad += !ok;
			}
		}
		rot++;
		free(sa); free(sb);
	}
	{ // one thread, 16 M samples of 0 against 255
		const size_t n = (size_t)4096 * 4096;
		uint8_t *sa = (uint8_t *)malloc(n), *sb = (uint8_t *)malloc(n);
		if (!sa || !sb) return 2;
		memset(sa, 0, n); memset(sb, 255, n);
		E264View v;
		for (int p = 0; p < 3; p++) v.plane[p] = (E264PlaneView){0, 4096, 4096, 4096};
		E264PlaneDiff got[3];
		const E264PlaneDiff want = {255ull << 24, 65025ull << 24, 1u << 24, 0, 255, 0};
		run_grid(v, sa, n, v, sb, n, 1, got);
		cases++;
		bool ok = true;
		for (int p = 0; p < 3; p++) ok = ok && same(got[p], want);
		if (!ok) fprintf(stderr, "4096 x 4096, 0 against 255, one thread: sad %llu sse %llu count %u first %u max %u\n", (unsigned long long)got[0].sad, (unsigned long long)got[0].sse,
			got[0].count, got[0].first, got[0].max);
		bad += !ok;
		free(sa); free(sb);
	}
	printf("diff_asan: %lu cases, %lu wrong\n", cases, bad);
	return bad ? 1 : 0;
}
