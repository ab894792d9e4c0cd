/*
 * edge264_hist.h -- the histogram record of include/edge264_hip.h (version 1) on the host: what e264hip_frame_hist,
 * e264hip_hist_batch and e264front_frame_hist compute on the device, for a caller that holds the same plane in host
 * memory (the CPU decoder's Edge264Frames: samples[k], stride_Y / stride_C, cropped width and height), and the
 * arithmetic on the 256 bins that the device leaves to the host.  Plain C, inline, no dependency.
 *
 *     bin[v] = the number of samples of the plane equal to v, v in 0..255
 *
 * Exact for planes of up to 65535 x 65535 samples (a bin < 2^32; sum < 2^40 and sum2 < 2^48 are kept in 64 bits).
 */
#ifndef EDGE264_HIST_H
#define EDGE264_HIST_H

#include <stddef.h>
#include <stdint.h>

#define EDGE264_HIST_VERSION 1 /* = E264_HIST_VERSION */

/* count = sum bin[v]; min, max = the smallest and largest v with bin[v] != 0 (255 and 0 for an empty histogram);
 * sum = sum v bin[v]; sum2 = sum v^2 bin[v].  mean = sum / count, variance = sum2 / count - mean^2. */
typedef struct { uint32_t count, min, max, zero; uint64_t sum, sum2; } E264HistStats;

/* THE DEFINITION: one plane of w x h samples, rows `stride` bytes apart */
static inline void e264_hist_plane(const uint8_t *s, size_t stride, unsigned w, unsigned h, uint32_t bin[256])
{
	unsigned x, y;
	for (x = 0; x < 256; x++) bin[x] = 0;
	for (y = 0; y < h; y++)
		for (x = 0; x < w; x++)
			bin[s[y * stride + x]]++;
}

static inline void e264_hist_stats(const uint32_t bin[256], E264HistStats *out)
{
	unsigned v;
	out->count = 0; out->min = 255; out->max = 0; out->zero = 0;
	out->sum = out->sum2 = 0;
	for (v = 0; v < 256; v++) {
		if (!bin[v]) continue;
		if (!out->count) out->min = v; /* (v counts up: the first occupied bin) */
		out->max = v;
		out->count += bin[v];
		out->sum += (uint64_t)v * bin[v];
		out->sum2 += (uint64_t)(v * v) * bin[v];
	}
}

/* the smallest v with at least num / den of the samples at or below it: (bin[0] + .. + bin[v]) * den >= count * num.  num = 0 gives 0 and
 * num = den the largest occupied v; 0 for an empty histogram; den = 0 or num > den give 255 where no v satisfies it.  (count * num < 2^64 for
 * num < 2^32.) */
static inline unsigned e264_hist_quantile(const uint32_t bin[256], uint32_t num, uint32_t den)
{
	uint64_t count = 0, below = 0;
	unsigned v;
	for (v = 0; v < 256; v++) count += bin[v];
	for (v = 0; v < 255; v++) {
		below += bin[v];
		if (below * den >= count * num) break;
	}
	return v;
}

#endif
