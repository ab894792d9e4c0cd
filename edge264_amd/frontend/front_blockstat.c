/*
 * front_blockstat.c -- e264front_frame_blockstat: the block statistics map (include/edge264_hip.h, version E264_BLOCKSTAT_VERSION;
 * include/edge264_blockstat.h computes the same on the host) of a frame edge264_get_frame has handed out, computed ON THE DEVICE from the picture
 * where it lies in HBM.
 *
 * Built into edge264_amd/libedge264_frontdigest.so beside front_digest.c, front_preview.c, front_diff.c, front_hist.c and front_blockdiff.c, for the
 * reasons given in the first, and through the same bindings (front_bind.h): e264front_digest_use serves all six.  The view is built exactly as
 * e264front_frame_digest builds it, so cropping and the second MVC view need nothing special, and it works with e264front_set_download(0): nothing is
 * read back but the map, 16 bytes per block.
 */
#include <errno.h>

#include "front_bind.h"
#include "edge264_blockstat.h"

/* out = the map Y | Cb | Cr (each plane bh x bw records of 16 bytes, tight) of the base view (view 0, fr->samples) or of the second MVC view (view 1,
 * fr->samples_mvc) of a frame edge264_get_frame has just handed out, in blocks of 1 << log2_block (3 .. 6); dims (may be NULL) = bw, bh of Y, Cb, Cr.
 * At most cap bytes are written.  Blocks until the kernels that write the picture and the block statistics kernel behind them have run.
 * 0; EINVAL (a null argument, no such view, log2_block outside 3..6, a plane that belongs to no frame of this decoder, a decoder without device; from
 * the back end, with a text in e264hip_last_error: cap smaller than the map); ENODEV (the front library or the back end is not to be found, or lacks
 * an entry point); or another error of the back end. */
PUBLIC int e264front_frame_blockstat(Edge264Decoder *dec, const Edge264Frame *fr, int view, int log2_block, void *out, size_t cap, uint16_t dims[6])
{
	if (!dec || !fr || !out || (view != 0 && view != 1) || log2_block < 3 || log2_block > 6) return EINVAL;
	int r = e264front_bind_once();
	if (r) return r;
	E264Stream *s;
	E264View v;
	int slot;
	if ((r = e264front_view_of(dec, fr, view, &s, &slot, &v))) return r;
	if ((r = e264front_bind.frame_blockstat(s, slot, &v, log2_block, out, cap))) return r;
	if (dims)
		for (int p = 0; p < 3; p++) {
			unsigned bw, bh;
			e264_blockstat_dims(v.plane[p].width, v.plane[p].height, log2_block, &bw, &bh); /* (the back end has accepted the view and the block size) */
			dims[2 * p] = (uint16_t)bw; dims[2 * p + 1] = (uint16_t)bh;
		}
	return 0;
}
