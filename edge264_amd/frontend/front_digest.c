/*
 * front_digest.c -- e264front_frame_digest: the digest (include/edge264_hip.h, version E264_DIGEST_VERSION; include/edge264_digest.h computes the
 * same on the host) of a frame edge264_get_frame has handed out, computed ON THE DEVICE from the picture where it lies in HBM.
 *
 * Built into edge264_amd/libedge264_frontdigest.so, a small library beside libedge264_hipfront.so, and NOT into that library: the front library
 * proper is compiled from the reference's sources, so a machine without the reference tree cannot rebuild it and runs whatever copy it was
 * given (edge264_amd/frontend/Makefile installs the one oracle/_ref holds).  Nothing here needs the decoder's internals: the slot, the
 * stream and the device address behind a plane pointer are what the front library has exported since decode-to-device exists
 * (e264front_slot_of, e264front_stream, e264front_device_samples), the rest is the back end's C ABI.  So this file builds on every machine,
 * from this repository alone, and works with any front library that has those three entry points.
 *
 * The view is what the frame says: plane pointers (their offsets in the slot = e264front_device_samples - e264hip_frame_device_ptr: same
 * offsets on the host and on the device), strides, cropped widths and heights -- cropping and the second MVC view need nothing special.  It
 * works with e264front_set_download(0): nothing is read back but the 24 bytes.
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "front_bind.h"

struct E264FrontBind e264front_bind = {ENODEV, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL};
#define g e264front_bind
static pthread_once_t g_once = PTHREAD_ONCE_INIT;

/* the library `name` that lies beside this one */
static void *open_sibling(const char *name)
{
	Dl_info info;
	char buf[4096];
	if (!dladdr((void *)open_sibling, &info) || !info.dli_fname) return NULL;
	snprintf(buf, sizeof(buf), "%s", info.dli_fname);
	char *s = strrchr(buf, '/');
	if (!s) return NULL;
	snprintf(s, sizeof(buf) - (size_t)(s - buf), "/%s", name);
	return dlopen(buf, RTLD_NOW | RTLD_LOCAL); /* (the instance the caller has loaded, if it has: one per file) */
}

static void *g_front, *g_hip; /* e264front_digest_use: the caller's own handles */

static void bind_all(void)
{
	/* the front library: the caller's handle; else the one the program is linked against or has loaded for all to see; else the one beside this library */
	void *fl = g_front ? g_front : dlsym(RTLD_DEFAULT, "e264front_device_samples") ? RTLD_DEFAULT : open_sibling("libedge264_hipfront.so");
	/* the back end: the caller's handle; else found as the front library finds it (E264_HIP_LIB, else its sibling) */
	const char *path = getenv("E264_HIP_LIB");
	void *hl = g_hip ? g_hip : path ? dlopen(path, RTLD_NOW | RTLD_LOCAL) : open_sibling("libedge264_hip.so");
	if (!fl || !hl) return;
	*(void **)&g.stream = dlsym(fl, "e264front_stream");
	*(void **)&g.device_samples = dlsym(fl, "e264front_device_samples");
	*(void **)&g.slot_of = dlsym(fl, "e264front_slot_of");
	*(void **)&g.frame_device_ptr = dlsym(hl, "e264hip_frame_device_ptr");
	*(void **)&g.frame_digest = dlsym(hl, "e264hip_frame_digest");
	*(void **)&g.preview_bytes = dlsym(hl, "e264hip_preview_bytes");
	*(void **)&g.frame_preview = dlsym(hl, "e264hip_frame_preview");
	*(void **)&g.frame_diff = dlsym(hl, "e264hip_frame_diff");
	*(void **)&g.frame_hist = dlsym(hl, "e264hip_frame_hist");
	*(void **)&g.frame_blockdiff = dlsym(hl, "e264hip_frame_blockdiff");
	*(void **)&g.frame_blockstat = dlsym(hl, "e264hip_frame_blockstat");
	if (g.stream && g.device_samples && g.slot_of && g.frame_device_ptr && g.frame_digest && g.preview_bytes && g.frame_preview && g.frame_diff && g.frame_hist && g.frame_blockdiff && g.frame_blockstat) g.err = 0;
}

int e264front_bind_once(void)
{
	pthread_once(&g_once, bind_all);
	return g.err;
}

/* A program that has loaded the front library and the back end itself (dlopen: a build of the front library that lies elsewhere, a variant of the back
 * end) hands over its two handles BEFORE the first e264front_frame_digest, e264front_frame_preview (front_preview.c), e264front_frame_diff (front_diff.c), e264front_frame_hist (front_hist.c), e264front_frame_blockdiff (front_blockdiff.c) or e264front_frame_blockstat (front_blockstat.c), so that the decoders it
 * passes meet the instance that made them.  Without this call the libraries are found as bind_all says.  0, or EINVAL (a null handle) / EALREADY (the first digest, preview, diff, histogram, block difference map or block statistics map has been asked for). */
PUBLIC int e264front_digest_use(void *front_lib, void *hip_lib)
{
	if (!front_lib || !hip_lib) return EINVAL;
	if (!g.err || g_front) return EALREADY;
	g_front = front_lib; g_hip = hip_lib;
	return 0;
}

int e264front_view_of(Edge264Decoder *dec, const Edge264Frame *fr, int view, E264Stream **stream, int *slot_out, E264View *v)
{
	E264Stream *s = (E264Stream *)g.stream(dec);
	if (!s) return EINVAL;
	const uint8_t *const *pl = view ? fr->samples_mvc : fr->samples;
	int slot = -1;
	for (int i = 0; i < 3; i++) { /* the three planes of a view lie in one slot */
		const int sl = pl[i] ? g.slot_of(dec, pl[i]) : -1;
		if (sl < 0 || (i && sl != slot)) return EINVAL;
		slot = sl;
	}
	/* plane 0's offset in the slot from its device address (one call, which also waits for the kernels that write the picture -- the lane's order
	 * would do, but the front library exports no other road to the offset); the other planes lie at the same distances on the host and on the device */
	const uint8_t *base = (const uint8_t *)g.frame_device_ptr(s, slot), *d0 = (const uint8_t *)g.device_samples(dec, pl[0]);
	if (!base || !d0 || d0 < base) return EINVAL;
	for (int i = 0; i < 3; i++) {
		const int64_t off = (int64_t)(d0 - base) + (int64_t)(pl[i] - pl[0]);
		if (off < 0 || off > (int64_t)UINT32_MAX) return EINVAL;
		v->plane[i] = (E264PlaneView){(uint32_t)off, (uint32_t)(uint16_t)(i ? fr->stride_C : fr->stride_Y), (uint16_t)(i ? fr->width_C : fr->width_Y),
			(uint16_t)(i ? fr->height_C : fr->height_Y)};
	}
	*stream = s; *slot_out = slot;
	return 0;
}

/* out[0..2] = the Y, Cb, Cr digests of the base view (view 0, fr->samples) or of the second MVC view (view 1, fr->samples_mvc) of a frame
 * edge264_get_frame has just handed out.  Blocks until the kernels that write the picture and the digest kernel behind them have run.
 * 0; EINVAL (a null argument, no such view, a plane that belongs to no frame of this decoder, a decoder without device); ENODEV (the front
 * library or the back end is not to be found, or lacks an entry point); or the back end's error (e264hip_last_error). */
PUBLIC int e264front_frame_digest(Edge264Decoder *dec, const Edge264Frame *fr, int view, uint64_t out[3])
{
	if (!dec || !fr || !out || (view != 0 && view != 1)) return EINVAL;
	int r = e264front_bind_once();
	if (r) return r;
	E264Stream *s;
	E264View v;
	int slot;
	if ((r = e264front_view_of(dec, fr, view, &s, &slot, &v))) return r;
	return g.frame_digest(s, slot, &v, out);
}
