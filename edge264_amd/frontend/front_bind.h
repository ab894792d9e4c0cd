/*
 * front_bind.h -- internal to libedge264_frontdigest.so (front_digest.c, front_preview.c, front_diff.c, front_hist.c, front_blockdiff.c, front_blockstat.c): the entry points of the front library and of the back end
 * the four files work through, bound once for all (front_digest.c; e264front_digest_use names the libraries), and the view a frame's planes make
 * in their slot.  Nothing here is exported.
 */
#ifndef E264_FRONT_BIND_H
#define E264_FRONT_BIND_H
#include <stddef.h>
#include <stdint.h>
#include "edge264_hip.h"

#define PUBLIC __attribute__((visibility("default")))
#define HIDDEN __attribute__((visibility("hidden")))

typedef struct Edge264Decoder Edge264Decoder;
/* edge264.h:45-62 (layout restated, as edge264_amd/driver/e264_multi.cpp does; the header itself is not part of this repository) */
typedef struct Edge264Frame {
	const uint8_t *samples[3];
	const uint8_t *samples_mvc[3];
	const uint8_t *mb_errors;
	int8_t bit_depth_Y, bit_depth_C;
	int16_t width_Y, width_C, height_Y, height_C, stride_Y, stride_C, stride_mb;
	int32_t FrameId, FrameId_mvc;
	int16_t frame_crop_offsets[4];
	void *return_arg;
} Edge264Frame;

struct E264FrontBind {
	int err; /* 0 once everything below is bound */
	void *(*stream)(Edge264Decoder *);
	void *(*device_samples)(Edge264Decoder *, const void *);
	int (*slot_of)(Edge264Decoder *, const void *);
	void *(*frame_device_ptr)(E264Stream *, int);
	int (*frame_digest)(E264Stream *, int, const E264View *, uint64_t *);
	size_t (*preview_bytes)(const E264View *, int, uint16_t *);
	int (*frame_preview)(E264Stream *, int, const E264View *, int, void *, size_t);
	int (*frame_diff)(E264Stream *, int, const E264View *, E264Stream *, int, const E264View *, E264Diff *);
	int (*frame_hist)(E264Stream *, int, const E264View *, E264Hist *);
	int (*frame_blockdiff)(E264Stream *, int, const E264View *, E264Stream *, int, const E264View *, int, void *, size_t);
	int (*frame_blockstat)(E264Stream *, int, const E264View *, int, void *, size_t);
};
extern HIDDEN struct E264FrontBind e264front_bind;

/* binds e264front_bind on the first call; 0, or ENODEV (the front library or the back end is not to be found, or lacks an entry point) */
HIDDEN int e264front_bind_once(void);
/* the stream, the slot and the view of the base view (view 0, fr->samples) or the second MVC view (view 1, fr->samples_mvc) of a frame edge264_get_frame
 * has handed out; waits for the kernels that write the picture.  0, or EINVAL (no such view, a plane that belongs to no frame of this decoder, a decoder
 * without device).  Call e264front_bind_once first. */
HIDDEN int e264front_view_of(Edge264Decoder *dec, const Edge264Frame *fr, int view, E264Stream **s, int *slot, E264View *v);
#endif
