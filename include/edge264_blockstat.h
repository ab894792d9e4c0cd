/*
 * edge264_blockstat.h -- the block statistics map of include/edge264_hip.h (version 1) on the host: what e264hip_frame_blockstat,
 * e264hip_blockstat_batch and e264front_frame_blockstat compute on the device, for a caller that holds the same plane in host
 * memory (the CPU decoder's Edge264Frames: samples[k], stride_Y / stride_C, cropped width and height) and wants to know
 * what to expect.  Plain C, inline, no dependency.
 *
 *     k = 3 .. 6      b = 1 << k      bw = (w + b - 1) >> k      bh = (h + b - 1) >> k
 *     record (Y, X), over the samples s(y, x) with  y in [b Y, min(b Y + b, h)),  x in [b X, min(b X + b, w)):
 *         sum = sum s      sumsq = sum s^2
 *         gh = sum |s(y, x + 1) - s(y, x)|  over those with x + 1 < w      gv = sum |s(y + 1, x) - s(y, x)|  over those with y + 1 < h
 *
 * A pair belongs to the block of its left (gh) or top (gv) sample, also where the other sample lies in the next block; a pair that would
 * leave the plane does not exist.  Nothing is clamped or replicated.  Exact: a block has at most 4096 samples, so sum, gh and
 * gv <= 4096 * 255 < 2^21 and sumsq <= 4096 * 255^2 < 2^29.  With n the block's sample count, mean = sum / n,
 * variance = (n sumsq - sum^2) / n^2, and n sumsq == sum^2 (in 64 bits) <=> the block is flat.
 */
#ifndef EDGE264_BLOCKSTAT_H
#define EDGE264_BLOCKSTAT_H

#include <stddef.h>
#include <stdint.h>

#define EDGE264_BLOCKSTAT_VERSION 1 /* = E264_BLOCKSTAT_VERSION */
#ifndef E264_BLOCKSTAT_VERSION
typedef struct { uint32_t sum, sumsq, gh, gv; } E264BlockStat; /* as in edge264_hip.h */
#endif

/* bw, bh of a plane of w x h samples at block size 1 << k; 0 (and nothing stored) for k outside 3..6 or a plane without samples, else 1 */
static inline int e264_blockstat_dims(unsigned w, unsigned h, int k, unsigned *bw, unsigned *bh)
{
	if (k < 3 || k > 6 || w < 1 || h < 1) return 0;
	*bw = (w + (1u << k) - 1) >> k;
	*bh = (h + (1u << k) - 1) >> k;
	return 1;
}

/* one plane: w x h samples, rows stride bytes apart; out: bh rows of bw records, tight.  k outside 3..6 or an empty plane: nothing is done */
static inline void e264_blockstat_plane(const uint8_t *s, size_t stride, unsigned w, unsigned h, int k, E264BlockStat *out)
{
	unsigned bw, bh, x, y, i;
	if (!e264_blockstat_dims(w, h, k, &bw, &bh)) return;
	for (i = 0; i < bw * bh; i++) out[i].sum = out[i].sumsq = out[i].gh = out[i].gv = 0;
	for (y = 0; y < h; y++)
		for (x = 0; x < w; x++) {
			const unsigned v = s[y * stride + x];
			E264BlockStat *r = &out[(size_t)(y >> k) * bw + (x >> k)];
			r->sum += v;
			r->sumsq += v * v;
			if (x + 1 < w) { const unsigned t = s[y * stride + x + 1]; r->gh += v > t ? v - t : t - v; }
			if (y + 1 < h) { const unsigned t = s[(y + 1) * stride + x]; r->gv += v > t ? v - t : t - v; }
		}
}

#endif
