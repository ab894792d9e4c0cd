/*
 * edge264_digest.h -- the picture digest of include/edge264_hip.h (version 1) on the host: what e264hip_frame_digest,
 * e264hip_digest_batch and e264front_frame_digest compute on the device, for a caller that holds the same plane in host
 * memory (the CPU decoder's Edge264Frame: samples[k], stride_Y / stride_C, cropped width and height) and wants to know what
 * to expect.  Plain C, inline, no dependency.
 *
 *     fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16      (mod 2^32)
 *     K(i) = fmix32(i) | 1
 *     D    = sum over i = y * w + x of (s[y][x] + 1) * K(i)                                       (mod 2^64)
 *
 * NOT cryptographic: it tells a wrong sample from a right one, not an adversary from a friend.
 */
#ifndef EDGE264_DIGEST_H
#define EDGE264_DIGEST_H

#include <stddef.h>
#include <stdint.h>

#define EDGE264_DIGEST_VERSION 1 /* = E264_DIGEST_VERSION */

static inline uint32_t e264_digest_fmix32(uint32_t h)
{
	h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
	return h;
}

/* one plane: w x h samples, rows `stride` bytes apart */
static inline uint64_t e264_digest_plane(const uint8_t *p, size_t stride, unsigned w, unsigned h)
{
	uint64_t d = 0;
	uint32_t i = 0;
	unsigned x, y;
	for (y = 0; y < h; y++)
		for (x = 0; x < w; x++, i++)
			d += (uint64_t)(p[(size_t)y * stride + x] + 1u) * (e264_digest_fmix32(i) | 1u);
	return d;
}

#endif
