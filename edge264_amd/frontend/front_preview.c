/*
 * front_preview.c -- e264front_frame_preview: the reduced preview (include/edge264_hip.h, version E264_PREVIEW_VERSION; include/edge264_preview.h
 * computes the same on the host) of a frame edge264_get_frame has handed out, computed ON THE DEVICE from the picture where it lies in HBM.
 *
 * Built into edge264_amd/libedge264_frontdigest.so beside front_digest.c, for the reasons given there, and through the same bindings (front_bind.h):
 * e264front_digest_use serves both.  The view is built exactly as e264front_frame_digest builds it, so cropping and the second MVC view need nothing
 * special, and it works with e264front_set_download(0): nothing is read back but the preview, 1/4, 1/16 or 1/64 of the picture's bytes.
 */
#include <errno.h>

#include "front_bind.h"

/* out = the preview Y | Cb | Cr (each plane tight) of the base view (view 0) or the second MVC view (view 1) of a frame edge264_get_frame has just
 * handed out, reduced by 1 << log2_factor (1, 2 or 3) in each direction; dims (may be NULL) = ow, oh of Y, Cb, Cr.  At most cap bytes are written.
 * Blocks until the kernels that write the picture and the preview kernel behind them have run.
 * 0; EINVAL (a null argument, no such view, log2_factor outside 1..3, cap smaller than the preview, a plane that belongs to no frame of this
 * decoder, a decoder without device); ENODEV (the front library or the back end is not to be found, or lacks an entry point); or the back end's
 * error (e264hip_last_error). */
PUBLIC int e264front_frame_preview(Edge264Decoder *dec, const Edge264Frame *fr, int view, int log2_factor, void *out, size_t cap, uint16_t dims[6])
{
	if (!dec || !fr || !out || (view != 0 && view != 1) || log2_factor < 1 || log2_factor > 3) return EINVAL;
	int r = e264front_bind_once();
	if (r) return r;
	E264Stream *s;
	E264View v;
	int slot;
	if ((r = e264front_view_of(dec, fr, view, &s, &slot, &v))) return r;
	if (!e264front_bind.preview_bytes(&v, log2_factor, dims)) return EINVAL;
	return e264front_bind.frame_preview(s, slot, &v, log2_factor, out, cap);
}
