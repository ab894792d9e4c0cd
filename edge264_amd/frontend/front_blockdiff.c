/*
 * front_blockdiff.c -- e264front_frame_blockdiff: the block difference map (include/edge264_hip.h, version E264_BLOCKDIFF_VERSION;
 * include/edge264_blockdiff.h computes the same on the host) of two frames edge264_get_frame has handed out, computed ON THE DEVICE from the two
 * pictures where they lie in HBM.
 *
 * Built into edge264_amd/libedge264_frontdigest.so beside front_digest.c, front_preview.c, front_diff.c and front_hist.c, for the reasons given in the
 * first, and through the same bindings (front_bind.h): e264front_digest_use serves all five.  Each side's view is built exactly as
 * e264front_frame_digest builds it, so cropping and the second MVC view need nothing special, and it works with e264front_set_download(0): nothing is
 * read back but the map, 8 bytes per block.
 *
 * Both frames must still be the caller's when the call is made, as for e264front_frame_diff: in practice one of them was fetched with borrow = 1 (and
 * goes back with edge264_return_frame after the comparison), or both were fetched between two edge264_decode_NAL calls.
 */
#include <errno.h>

#include "front_bind.h"
#include "edge264_blockdiff.h"

/* out = the map Y | Cb | Cr (each plane bh x bw records of 8 bytes, tight) of the base view (view 0) or the second MVC view (view 1) of frame_a of dec_a
 * against that of frame_b of dec_b, in blocks of 1 << log2_block (3 .. 6); dims (may be NULL) = bw, bh of Y, Cb, Cr.  At most cap bytes are written.
 * dec_a == dec_b is the common case (consecutive output frames of one stream); two decoders must share a device and a compute lane.
 * Blocks until the kernels that write the two pictures and the block difference kernel behind them have run.
 * 0; EINVAL (a null argument, no such view, log2_block outside 3..6, a plane that belongs to no frame of its decoder, a decoder without device; from the
 * back end, with a text in e264hip_last_error: cap smaller than the map, two devices or lanes, planes of the two frames that differ in size); ENODEV (the
 * front library or the back end is not to be found, or lacks an entry point); or another error of the back end. */
PUBLIC int e264front_frame_blockdiff(Edge264Decoder *dec_a, const Edge264Frame *frame_a, int view_a, Edge264Decoder *dec_b, const Edge264Frame *frame_b, int view_b,
	int log2_block, void *out, size_t cap, uint16_t dims[6])
{
	if (!dec_a || !frame_a || !dec_b || !frame_b || !out || (view_a != 0 && view_a != 1) || (view_b != 0 && view_b != 1) || log2_block < 3 || log2_block > 6) return EINVAL;
	int r = e264front_bind_once();
	if (r) return r;
	E264Stream *sa, *sb;
	E264View va, vb;
	int slot_a, slot_b;
	if ((r = e264front_view_of(dec_a, frame_a, view_a, &sa, &slot_a, &va)) || (r = e264front_view_of(dec_b, frame_b, view_b, &sb, &slot_b, &vb))) return r;
	if ((r = e264front_bind.frame_blockdiff(sa, slot_a, &va, sb, slot_b, &vb, log2_block, out, cap))) return r;
	if (dims)
		for (int p = 0; p < 3; p++) {
			unsigned bw, bh;
			e264_blockdiff_dims(va.plane[p].width, va.plane[p].height, log2_block, &bw, &bh); /* (the back end has accepted the view and the block size) */
			dims[2 * p] = (uint16_t)bw; dims[2 * p + 1] = (uint16_t)bh;
		}
	return 0;
}
