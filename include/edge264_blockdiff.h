/*
 * edge264_blockdiff.h -- the block difference map of include/edge264_hip.h (version 1) on the host: what e264hip_frame_blockdiff,
 * e264hip_blockdiff_batch and e264front_frame_blockdiff compute on the device, for a caller that holds the same two planes in host
 * memory (the CPU decoder's Edge264Frames: samples[k], stride_Y / stride_C, cropped width and height) and wants to know
 * what to expect.  Plain C, inline, no dependency.
 *
 *     k = 3 .. 6      b = 1 << k      bw = (w + b - 1) >> k      bh = (h + b - 1) >> k
 *     record (Y, X):  sad = sum |a - b|,  sse = sum (a - b)^2  over  y in [b Y, min(b Y + b, h)),  x in [b X, min(b X + b, w))
 *
 * Samples outside the plane do not count.  Exact: a block has at most 4096 samples, so sad <= 4096 * 255 and sse <= 4096 * 255^2 < 2^32.
 * Regional PSNR = 10 log10(255^2 n / sse) for the n samples of the block, infinite for sse == 0.
 */
#ifndef EDGE264_BLOCKDIFF_H
#define EDGE264_BLOCKDIFF_H

#include <stddef.h>
#include <stdint.h>

#define EDGE264_BLOCKDIFF_VERSION 1 /* = E264_BLOCKDIFF_VERSION */
#ifndef E264_BLOCKDIFF_VERSION
typedef struct { uint32_t sad, sse; } E264BlockDiff; /* as in edge264_hip.h */
#endif

/* bw, bh of a plane of w x h samples at block size 1 << k; 0 (and nothing stored) for k outside 3..6 or a plane without samples, else 1 */
static inline int e264_blockdiff_dims(unsigned w, unsigned h, int k, unsigned *bw, unsigned *bh)
{
	if (k < 3 || k > 6 || w < 1 || h < 1) return 0;
	*bw = (w + (1u << k) - 1) >> k;
	*bh = (h + (1u << k) - 1) >> k;
	return 1;
}

/* one plane of A against the same plane of B: w x h samples each, rows stride_a / stride_b bytes apart; out: bh rows of bw records, tight.
 * k outside 3..6 or an empty plane: nothing is done */
static inline void e264_blockdiff_plane(const uint8_t *a, size_t stride_a, const uint8_t *b, size_t stride_b, unsigned w, unsigned h, int k, E264BlockDiff *out)
{
	unsigned bw, bh, x, y, i;
	if (!e264_blockdiff_dims(w, h, k, &bw, &bh)) return;
	for (i = 0; i < bw * bh; i++) out[i].sad = out[i].sse = 0;
	for (y = 0; y < h; y++)
		for (x = 0; x < w; x++) {
			const unsigned s = a[y * stride_a + x], t = b[y * stride_b + x], d = s > t ? s - t : t - s;
			E264BlockDiff *r = &out[(size_t)(y >> k) * bw + (x >> k)];
			r->sad += d;
			r->sse += d * d;
		}
}

#endif
