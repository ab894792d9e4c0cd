/*
 * edge264_preview.h -- the reduced preview of include/edge264_hip.h (version 1) on the host: what e264hip_frame_preview,
 * e264hip_preview_batch and e264front_frame_preview compute on the device, for a caller that holds the same plane in host
 * memory (the CPU decoder's Edge264Frame: samples[k], stride_Y / stride_C, cropped width and height) and wants to know what
 * to expect.  Plain C, inline, no dependency.
 *
 *     k = 1, 2, 3      f = 1 << k      ow = (w + f - 1) >> k      oh = (h + f - 1) >> k
 *     P[Y][X] = (sum over dy < f, dx < f of s[min(f Y + dy, h - 1)][min(f X + dx, w - 1)]  +  (1 << (2 k - 1))) >> 2 k
 *
 * A box filter: a box that leaves the plane repeats its last column or row, the divisor is always f * f, everything is exact
 * in integers (a box sum stays below 2^14).
 */
#ifndef EDGE264_PREVIEW_H
#define EDGE264_PREVIEW_H

#include <stddef.h>
#include <stdint.h>

#define EDGE264_PREVIEW_VERSION 1 /* = E264_PREVIEW_VERSION */

/* the preview's size for a plane of w x h samples; 0 (and nothing written) for k outside 1..3 or a plane without samples */
static inline int e264_preview_dims(unsigned w, unsigned h, int k, unsigned *ow, unsigned *oh)
{
	if (k < 1 || k > 3 || w < 1 || h < 1) return 0;
	*ow = (w + (1u << k) - 1) >> k;
	*oh = (h + (1u << k) - 1) >> k;
	return 1;
}

/* one plane: w x h samples, rows `stride` bytes apart, into ow x oh bytes, rows `dst_stride` bytes apart */
static inline void e264_preview_plane(const uint8_t *src, size_t stride, unsigned w, unsigned h, int k, uint8_t *dst, size_t dst_stride)
{
	unsigned ow, oh, X, Y, dx, dy;
	const unsigned f = 1u << k;
	if (!e264_preview_dims(w, h, k, &ow, &oh)) return;
	for (Y = 0; Y < oh; Y++)
		for (X = 0; X < ow; X++) {
			unsigned sum = 1u << (2 * k - 1);
			for (dy = 0; dy < f; dy++) {
				const unsigned y = f * Y + dy < h ? f * Y + dy : h - 1;
				for (dx = 0; dx < f; dx++)
					sum += src[(size_t)y * stride + (f * X + dx < w ? f * X + dx : w - 1)];
			}
			dst[(size_t)Y * dst_stride + X] = (uint8_t)(sum >> (2 * k));
		}
}

#endif
