/*
 * edge264_diff.h -- the difference record of include/edge264_hip.h (version 1) on the host: what e264hip_frame_diff,
 * e264hip_diff_batch and e264front_frame_diff compute on the device, for a caller that holds the same two planes in host
 * memory (the CPU decoder's Edge264Frames: samples[k], stride_Y / stride_C, cropped width and height) and wants to know
 * what to expect.  Plain C, inline, no dependency.
 *
 *     i = y * w + x      d_i = |a_i - b_i|
 *     sad = sum d_i    sse = sum d_i^2    count = #{i: d_i != 0}    max = max d_i    first = min {i: d_i != 0} or NONE    zero = 0
 *
 * Everything is exact in integers for planes of up to 65535 x 65535 samples (sad < 2^40, sse < 2^48, count < 2^32).
 * PSNR = 10 log10(255^2 w h / sse), infinite for sse == 0.
 */
#ifndef EDGE264_DIFF_H
#define EDGE264_DIFF_H

#include <stddef.h>
#include <stdint.h>

#define EDGE264_DIFF_VERSION 1 /* = E264_DIFF_VERSION */
#ifndef E264_DIFF_NONE
#define E264_DIFF_NONE 0xffffffffu
typedef struct { uint64_t sad, sse; uint32_t count, first, max, zero; } E264PlaneDiff; /* as in edge264_hip.h */
#endif

/* one plane of A against the same plane of B: w x h samples each, rows stride_a / stride_b bytes apart */
static inline void e264_diff_plane(const uint8_t *a, size_t stride_a, const uint8_t *b, size_t stride_b, unsigned w, unsigned h, E264PlaneDiff *out)
{
	unsigned x, y;
	out->sad = out->sse = 0;
	out->count = out->max = out->zero = 0;
	out->first = E264_DIFF_NONE;
	for (y = 0; y < h; y++)
		for (x = 0; x < w; x++) {
			const unsigned s = a[y * stride_a + x], t = b[y * stride_b + x], d = s > t ? s - t : t - s;
			if (!d) continue;
			out->sad += d;
			out->sse += d * d;
			if (out->count++ == 0) out->first = (uint32_t)(y * w + x);
			if (d > out->max) out->max = d;
		}
}

#endif
