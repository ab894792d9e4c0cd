/*
 * front_hist.c -- e264front_frame_hist: the histogram record (include/edge264_hip.h, version E264_HIST_VERSION; include/edge264_hist.h computes the
 * same on the host) of a frame edge264_get_frame has handed out, computed ON THE DEVICE from the picture where it lies in HBM.
 *
 * Built into edge264_amd/libedge264_frontdigest.so beside front_digest.c, front_preview.c and front_diff.c, for the reasons given in the first, and
 * through the same bindings (front_bind.h): e264front_digest_use serves all four.  The view is built exactly as e264front_frame_digest builds it, so
 * cropping and the second MVC view need nothing special, and it works with e264front_set_download(0): nothing is read back but the 3072 bytes.
 */
#include <errno.h>

#include "front_bind.h"

/* out = the record of the base view (view 0, fr->samples) or of the second MVC view (view 1, fr->samples_mvc) of a frame edge264_get_frame has just
 * handed out.  Blocks until the kernels that write the picture and the histogram kernel behind them have run.
 * 0; EINVAL (a null argument, no such view, a plane that belongs to no frame of this decoder, a decoder without device); ENODEV (the front
 * library or the back end is not to be found, or lacks an entry point); or the back end's error (e264hip_last_error). */
PUBLIC int e264front_frame_hist(Edge264Decoder *dec, const Edge264Frame *fr, int view, E264Hist *out)
{
	if (!dec || !fr || !out || (view != 0 && view != 1)) return EINVAL;
	int r = e264front_bind_once();
	if (r) return r;
	E264Stream *s;
	E264View v;
	int slot;
	if ((r = e264front_view_of(dec, fr, view, &s, &slot, &v))) return r;
	return e264front_bind.frame_hist(s, slot, &v, out);
}
