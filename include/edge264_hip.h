/*
 * edge264_hip.h -- C ABI of the MI355X macroblock-reconstruction back end
 * (libedge264_hip.so, built from edge264_amd/csrc/ with hipcc for gfx950).
 *
 * This is the drop-in boundary of BASELINE.json's north_star: everything that
 * touches the BITSTREAM (CAVLC/CABAC, mvpred, DPB bookkeeping) stays in the
 * edge264 C front end; everything that touches SAMPLES is behind these entry
 * points.  Plain pointers and sizes only -- what a C front end (or cgo / JNI /
 * ctypes) binds.  Each function names the reference interface it replaces
 * (/root/reference, file:line).  INTEGRATION.md shows the reference-side glue.
 *
 * Threading: a E264Device may be shared by threads; one E264Stream (= one
 * Edge264Decoder) is driven by one thread at a time, like the reference's
 * n_threads==0 mode (src/edge264_headers.c:1285-1286).
 * Errors: 0 or a positive errno value like the reference (src/edge264_internal.h:1259-1263):
 * ENOMEM (device/pinned allocation), EINVAL (bad packet/slot), EIO (HIP runtime failure),
 * ENODEV (no gfx950 device).  Nothing aborts.
 */
#ifndef EDGE264_HIP_H
#define EDGE264_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "edge264_cmd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct E264Device E264Device; /* one per GPU: compute lanes (HIP queues), upload / download queues, kernels */
typedef struct E264Stream E264Stream; /* one per decoder: device DPB slots + host mirrors */

/* ---- device ------------------------------------------------------------ */
/* Selected in edge264_alloc where the reference picks its ISA variant
 * (src/edge264.c:161-216): open once per GPU, share between decoders. */
int  e264hip_device_open(int ordinal, E264Device **out);
void e264hip_device_close(E264Device *dev);
int  e264hip_device_sync(E264Device *dev);
const char *e264hip_last_error(void);

/* ---- decoder-side objects ---------------------------------------------- */
int  e264hip_stream_open(E264Device *dev, E264Stream **out);
void e264hip_stream_close(E264Stream *s);
/* Compute lanes.  A device has E264_MAX_LANES HIP queues for kernels; a stream is bound to one (default 0) and everything
 * that touches its DPB is ordered there, like the frames of one Edge264Decoder are ordered by its task queue
 * (src/edge264_internal.h:396-400).  Streams of different lanes are independent (src/edge264_internal.h:144-151: no shared
 * state between decoders), so their submissions overlap on the GPU: the tile-parallel kernels of one lane use the compute
 * units the wavefront kernels of another leave idle.  All streams of one batch must share a lane.  Rebinding waits for
 * what the stream still has queued on its old lane. */
#define E264_MAX_LANES 4
int  e264hip_stream_bind_lane(E264Stream *s, int lane);

/* Frame memory.  Replaces Edge264AllocCb / Edge264FreeCb (edge264.h:42-43; called from
 * alloc_frame, src/edge264_headers.c:113-133): the samples of DPB slot `slot` live in
 * HBM; *host_mirror (pinned, samples_bytes) is what Edge264Frame.samples will point
 * into (src/edge264.c:385-387) once e264hip_frame_download has run. */
int  e264hip_frame_alloc(E264Stream *s, int slot, size_t samples_bytes, void **host_mirror);
void e264hip_frame_free(E264Stream *s, int slot);
/* "non-existing" frames of frame_num gaps (src/edge264_headers.c:1122-1144) and tests */
int  e264hip_frame_fill(E264Stream *s, int slot, int value);
int  e264hip_frame_upload(E264Stream *s, int slot, const void *src, size_t bytes);

/* Submit one coded frame.  Replaces the sample-writing half of the per-slice worker
 * (worker_loop, src/edge264_headers.c:450-603: every decode_intra / decode_inter / add_idct /
 * deblock_mb call issued by parse_slice_data, src/edge264_slice.c:1651-1849).  `packet` is a
 * host buffer (ideally from e264hip_packet_buffer, pinned); the call enqueues the H2D copy
 * and the kernels on the device queue and returns without waiting. */
int  e264hip_frame_submit(E264Stream *s, const void *packet, size_t bytes);
/* Pinned staging memory for the emitters, recycled when the copy has been consumed. */
void *e264hip_packet_buffer(E264Stream *s, size_t max_bytes);

/* Readiness test of edge264_get_frame (next_deblock_addr[pic]==INT_MAX, src/edge264.c:373)
 * becomes "the kernels that write this slot have completed". */
int  e264hip_frame_wait(E264Stream *s, int slot);
/* Copy the finished frame to its host mirror (what get_frame hands out). */
int  e264hip_frame_download(E264Stream *s, int slot, void *dst, size_t bytes);
/* Decode-to-device use (the consumer of the pictures is another GPU stage -- scaler, encoder, inference): the
 * HBM address of slot `slot` in the reference's frame layout (Edge264Frame: Y plane, then rows of Cb | Cr, strides as in the
 * packet header), valid until e264hip_frame_free; call e264hip_frame_wait first.  NULL when the slot is not allocated.  Nothing
 * crosses PCIe.  The reference has no counterpart (its frames are host memory, edge264.h:45-62). */
void *e264hip_frame_device_ptr(E264Stream *s, int slot);
/* edge264_flush (src/edge264.c:261-270): wait for what THIS stream has submitted, keep allocations.  (frame_alloc,
 * frame_free, stream_close and frame_download likewise never wait for other decoders' work: freed memory is parked and
 * recycled by the device object instead of hipFree'd, which would drain every queue.) */
int  e264hip_stream_flush(E264Stream *s);

/* ---- digests of decoded pictures, computed on the device ------------------------------------------------ */
/* Verifying a picture without reading it back (e264hip_frame_download moves the whole padded slot, 3.1 MB at 1080p): the device
 * reads the picture's samples where they lie and hands out three 64-bit numbers.  The reference has no counterpart (a test of it
 * hashes Edge264Frame's planes on the host, which include/edge264_digest.h's e264_digest_plane does in the same arithmetic).
 *
 * THE DIGEST, version E264_DIGEST_VERSION.  For one plane of w x h samples s[y][x], with i = y * w + x:
 *     fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16      (mod 2^32)
 *     K(i) = fmix32(i) | 1
 *     D    = sum over i of (s_i + 1) * K(i)                                                       (mod 2^64)
 * A picture's digest is three such values: Y, Cb, Cr, each plane indexed from 0 over its own (cropped) view, row-major.  The sum
 * commutes, so every split over lanes, waves and workgroups gives the same bits; one changed sample changes D (an odd K times a
 * difference below 256 is not 0 mod 2^64); the + 1 makes a plane of zeros depend on its size.  It is NOT cryptographic: it
 * detects decoding errors, not an adversary.
 *
 * WHERE A PICTURE LIES.  E264View is what an Edge264Frame says about a slot: plane pointers minus the slot's base, strides,
 * cropped widths and heights -- cropping, padded layouts and the second MVC view are all just other numbers.
 * e264hip_view_check (host only, like e264hip_packet_check: 0 or EINVAL with a text) accepts a view only if every plane has
 * width >= 1, height >= 1, stride >= width and offset + (height - 1) * stride + width <= slot_bytes, computed in 64 bits. */
typedef struct { uint32_t offset, stride; uint16_t width, height; } E264PlaneView; /* bytes from the slot's start; bytes between rows; samples */
typedef struct { E264PlaneView plane[3]; } E264View;                               /* Y, Cb, Cr */
#define E264_DIGEST_VERSION 1
int  e264hip_view_check(const E264View *v, size_t slot_bytes);
/* out[3 i .. 3 i + 2] = the digest of views[i] of slot slots[i] of streams[i]; e264hip_frame_digest is the batch of one.  Both
 * BLOCK until `out` (ordinary host memory) is filled.
 * Ordering: one kernel, queued on the streams' compute lane behind everything queued there -- a digest asked for right after
 *   e264hip_frame_submit, e264hip_submit_batch* or e264hip_frame_fill, with no wait between, sees that work's result.  All streams
 *   of a call belong to `dev` and share one lane, as for a submission (else EINVAL); a stream may appear more than once (the pass
 *   only reads).  The call waits for its own event, never for the device.
 * Lifetime: the call marks the lane as a fill does, so a slot freed while it runs stays parked behind it (e264hip_frame_free never
 *   hands memory back under a kernel); the caller drives the streams, as for a submission.
 * Errors: EINVAL (and nothing is queued) for a null pointer, n < 0, n > E264_DIGEST_MAX_BATCH, a slot out of range or not
 *   allocated, a view e264hip_view_check refuses for that slot's size; e264hip_last_error() names the cause.  n == 0 returns 0. */
#define E264_DIGEST_MAX_BATCH 4096
int  e264hip_frame_digest(E264Stream *s, int slot, const E264View *view, uint64_t out[3]);
int  e264hip_digest_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n, uint64_t *out);

/* ---- reduced previews of decoded pictures, computed on the device ---------------------------------------- */
/* A small picture of every stream (a monitoring wall, a scene-change or black-frame detector, a low-resolution inference stage) without
 * reading the full-size one back: the device reduces the picture where it lies by 2, 4 or 8 in each direction and hands out 1/4, 1/16 or
 * 1/64 of the bytes.  The reference has no counterpart (include/edge264_preview.h's e264_preview_plane does the same arithmetic on an
 * Edge264Frame's planes on the host).
 *
 * THE PREVIEW, version E264_PREVIEW_VERSION.  For one plane of w x h samples s[y][x] and a reduction k = log2_factor in {1, 2, 3}, f = 1 << k:
 *     ow = (w + f - 1) >> k          oh = (h + f - 1) >> k
 *     P[Y][X] = (sum over dy < f, dx < f of s[min(f Y + dy, h - 1)][min(f X + dx, w - 1)]  +  (1 << (2 k - 1))) >> 2 k
 * A box that leaves the view repeats the view's last column or row; the divisor is always f * f, so the result is exact in integers.  The
 * three planes of a view (E264View, above) are reduced independently, each over its own cropped view; the result stays 4:2:0, since
 * ceil(ceil(w / 2) / f) = ceil(ceil(w / f) / 2).  One picture's preview is Y | Cb | Cr, each plane tight (ow bytes per row): the sum of
 * ow_p * oh_p bytes.
 *
 * e264hip_preview_bytes (host only): that size, and in dims (may be NULL) ow, oh of Y, Cb, Cr; 0 for a null view, k outside 1..3 or a plane
 *   without samples.
 * e264hip_preview_batch: the preview of views[i] of slot slots[i] of streams[i] at out + i * pitch; only its e264hip_preview_bytes bytes there
 *   are written, the rest of a pitch is left as it was.  e264hip_frame_preview is the batch of one with pitch = cap.  Both BLOCK until `out`
 *   (ordinary host memory) is filled.
 * Ordering and lifetime are the digest's: one kernel, queued on the streams' compute lane behind everything queued there; all streams of a
 *   call belong to `dev` and share one lane; a stream may appear more than once; the call marks the lane as a fill does and waits for its own
 *   event, never for the device.
 * Errors: EINVAL (and nothing is queued) for a null pointer, n < 0, n > E264_PREVIEW_MAX_BATCH, k outside 1..3, a slot out of range or not
 *   allocated, streams of two lanes, a view e264hip_view_check refuses for that slot's size, pitch or cap smaller than a picture's preview,
 *   more than E264_PREVIEW_MAX_BYTES in one call; e264hip_last_error() names the cause.  n == 0 returns 0. */
#define E264_PREVIEW_VERSION 1
#define E264_PREVIEW_MAX_BATCH 4096
#define E264_PREVIEW_MAX_BYTES (1u << 28)   /* of one call: the sum of the pictures' previews, each rounded up to 16 */
size_t e264hip_preview_bytes(const E264View *v, int log2_factor, uint16_t dims[6]);
int  e264hip_frame_preview(E264Stream *s, int slot, const E264View *view, int log2_factor, void *out, size_t cap);
int  e264hip_preview_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n,
                           int log2_factor, void *out, size_t pitch);

/* ---- two decoded pictures compared on the device: the per-plane difference record ------------------------ */
/* How two pictures in HBM relate (consecutive output pictures of a stream for a freeze or scene-change detector, two renditions of one
 * content for PSNR, a picture whose digest did not match against the expected one) without reading either back.  The reference has no
 * counterpart (include/edge264_diff.h's e264_diff_plane does the same arithmetic on two Edge264Frames' planes on the host).
 *
 * THE DIFFERENCE RECORD, version E264_DIFF_VERSION.  For plane p of view A and of view B, both w x h samples, i = y * w + x, d_i = |a_i - b_i|:
 *     sad = sum of d_i      sse = sum of d_i^2      count = the number of i with d_i != 0      max = max d_i (0 for equal planes)
 *     first = the smallest i with d_i != 0, E264_DIFF_NONE where there is none (the largest index of a view is 65535^2 - 1 < E264_DIFF_NONE)
 *     zero = 0
 * Each plane is indexed from 0 over its own (cropped) view, row-major, as for the digest.  Everything is exact in integers for every view
 * e264hip_view_check accepts: count < 2^32, sad < 2^40, sse < 2^48.  Every member is a sum, a max or a min, so every split over lanes, waves
 * and workgroups, and every order in which workgroups finish, gives the same record.
 * PSNR is not part of the record: it is 10 log10(255^2 w h / sse), infinite for sse == 0 (edge264_amd/diff.py: psnr).
 *
 * e264hip_diff_batch: out[i] = views_a[i] of slot slots_a[i] of streams_a[i] against views_b[i] of slot slots_b[i] of streams_b[i];
 *   e264hip_frame_diff is the batch of one.  Both BLOCK until `out` (ordinary host memory) is filled.  A and B may be different streams, the same
 *   stream, even the same slot and view (the record is then all zero, with first = E264_DIFF_NONE).
 * Ordering: one kernel per call, whatever n, queued on the streams' compute lane behind everything queued there -- a diff asked for right after
 *   e264hip_frame_submit, e264hip_submit_batch*, e264hip_frame_fill or e264hip_frame_upload, with no wait between, sees that work's result.  All
 *   streams of a call, on both sides, belong to `dev` and share one lane, as for a submission (else EINVAL); a stream may appear more than once (the
 *   pass only reads).  The call waits for its own event, never for the device.
 * Lifetime: the call marks the lane as a fill does, so a slot freed while it runs stays parked behind it (e264hip_frame_free never hands memory
 *   back under a kernel); the caller drives the streams, as for a submission.
 * Errors: EINVAL (and nothing is queued, `out` is untouched) for a null pointer, n < 0, n > E264_DIFF_MAX_BATCH, a slot out of range or not allocated,
 *   streams of two devices or two lanes, a view e264hip_view_check refuses for its own slot's size (either side), plane p of A and of B differing in
 *   width or height for any p; e264hip_last_error() names the cause.  n == 0 returns 0.
 * e264hip_diff_check (host only, like e264hip_view_check): what the two calls ask of one pair of views and their slots' sizes; 0 or EINVAL with a text. */
typedef struct { uint64_t sad, sse; uint32_t count, first, max, zero; } E264PlaneDiff; /* 32 bytes */
typedef struct { E264PlaneDiff plane[3]; } E264Diff;                                    /* Y, Cb, Cr: 96 bytes */
#define E264_DIFF_VERSION 1
#define E264_DIFF_NONE 0xffffffffu
#define E264_DIFF_MAX_BATCH 4096
int  e264hip_diff_check(const E264View *view_a, size_t slot_bytes_a, const E264View *view_b, size_t slot_bytes_b);
int  e264hip_frame_diff(E264Stream *a, int slot_a, const E264View *view_a,
                        E264Stream *b, int slot_b, const E264View *view_b, E264Diff *out);
int  e264hip_diff_batch(E264Device *dev,
                        E264Stream *const *streams_a, const int *slots_a, const E264View *views_a,
                        E264Stream *const *streams_b, const int *slots_b, const E264View *views_b,
                        int n, E264Diff *out);

/* ---- histograms of decoded pictures, computed on the device ---------------------------------------------- */
/* The distribution of a picture's own sample values (black-frame, flash and fade detectors, exposure and clipping meters, histogram-distance
 * scene-cut detectors, auto-levels, entropy estimates) without reading the picture back: 3072 bytes come down instead of the picture.  A preview's
 * histogram is not the picture's -- a box filter removes the extremes a clipping or black-level meter looks for -- and the difference record says
 * nothing about levels.  The reference has no counterpart (include/edge264_hist.h's e264_hist_plane counts an Edge264Frame's planes on the host).
 *
 * THE HISTOGRAM RECORD, version E264_HIST_VERSION.  For plane p of a view (E264View, above: cropped, as for the digest):
 *     bin[p][v] = the number of samples of the plane equal to v, for v in 0..255
 * The record is exact: a view has at most 65535^2 < 2^32 samples per plane, so a bin cannot wrap, and the bins of a plane sum to width * height.
 * Every bin is a sum, so every split over lanes, waves and workgroups, and every order of arrival, gives the same record.  The bins are the WHOLE
 * record: count, min, max, sum, sum of squares, mean, variance and quantiles are arithmetic on 256 numbers and belong on the host
 * (include/edge264_hist.h: e264_hist_stats, e264_hist_quantile; edge264_amd/hist.py: stats, quantile, distance).
 *
 * e264hip_hist_batch: out[i] = the record of views[i] of slot slots[i] of streams[i]; e264hip_frame_hist is the batch of one.  Both BLOCK until `out`
 *   (ordinary host memory) is filled.
 * Ordering: one kernel per call, whatever n, queued on the streams' compute lane behind everything queued there -- a histogram asked for right after
 *   e264hip_frame_submit, e264hip_submit_batch*, e264hip_frame_fill or e264hip_frame_upload, with no wait between, sees that work's result.  All
 *   streams of a call belong to `dev` and share one lane, as for a submission (else EINVAL); a stream may appear more than once (the pass only
 *   reads).  The call waits for its own event, never for the device.
 * Lifetime: the call marks the lane as a fill does, so a slot freed while it runs stays parked behind it (e264hip_frame_free never hands memory
 *   back under a kernel); the caller drives the streams, as for a submission.
 * Errors: EINVAL (and nothing is queued, `out` is untouched) for a null pointer, n < 0, n > E264_HIST_MAX_BATCH, a slot out of range or not allocated,
 *   streams of two devices or two lanes, a view e264hip_view_check refuses for that slot's size; e264hip_last_error() names the cause.  n == 0
 *   returns 0.  e264hip_view_check is the whole validation of a view: there is no check export of the histogram's own. */
typedef struct { uint32_t bin[3][256]; } E264Hist;   /* Y, Cb, Cr: 3072 bytes */
#define E264_HIST_VERSION 1
#define E264_HIST_MAX_BATCH 4096
int  e264hip_frame_hist(E264Stream *s, int slot, const E264View *view, E264Hist *out);
int  e264hip_hist_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views, int n, E264Hist *out);

/* ---- WHERE two decoded pictures differ: the per-block difference map, computed on the device ------------- */
/* The difference record says how two pictures relate as a whole and names one sample; the map says where they differ and by how much, block by
 * block: which macroblocks of a picture whose digest did not match went wrong, motion masks and regional freeze detection (a picture that stands
 * still but for a clock or a ticker), regional PSNR of two renditions, regions of interest for a transcode or inference stage -- without reading
 * either picture back.  The reference has no counterpart (include/edge264_blockdiff.h's e264_blockdiff_plane does the same arithmetic on two
 * Edge264Frames' planes on the host).
 *
 * THE BLOCK DIFFERENCE MAP, version E264_BLOCKDIFF_VERSION.  k = log2_block in {3, 4, 5, 6}, b = 1 << k.  For plane p of view A and of view B, both
 * w x h samples:
 *     bw = (w + b - 1) >> k          bh = (h + b - 1) >> k
 *     record (Y, X) covers the samples y in [b Y, min(b Y + b, h)), x in [b X, min(b X + b, w)):  sad = sum |a - b|,  sse = sum (a - b)^2
 * Samples outside the view do not count: there is no clamping and no replication, a block at the right or bottom edge simply has fewer samples.
 * One pair's map is Y | Cb | Cr, each plane row-major bh x bw records, tight.  The three planes use the same b independently, each over its own
 * (cropped) view, as the preview does, so the result stays 4:2:0: a chroma block of b covers the area of a luma block of 2 b.
 * Everything is exact: a block has at most 64 x 64 = 4096 samples, so sad <= 4096 * 255 < 2^21 and sse <= 4096 * 255^2 = 266 342 400 < 2^32.
 * For every plane, the sum of sad over the map is E264PlaneDiff.sad of the same pair and the sum of sse its sse; and
 * sad == 0 <=> sse == 0 <=> the block's samples are equal.
 *
 * e264hip_blockdiff_bytes (host only): the map's size, and in dims (may be NULL) bw, bh of Y, Cb, Cr; 0 for a null view, k outside 3..6 or a plane
 *   without samples.
 * e264hip_blockdiff_batch: the map of views_a[i] of slot slots_a[i] of streams_a[i] against views_b[i] of slot slots_b[i] of streams_b[i] at
 *   out + i * pitch; only its e264hip_blockdiff_bytes bytes there are written, the rest of a pitch is left as it was.  e264hip_frame_blockdiff is the
 *   batch of one with pitch = cap.  Both BLOCK until `out` (ordinary host memory) is filled.  A and B may be different streams, the same stream, even
 *   the same slot and view (every record is then zero).
 * Ordering: one kernel per call, whatever n, queued on the streams' compute lane behind everything queued there -- a map asked for right after
 *   e264hip_frame_submit, e264hip_submit_batch*, e264hip_frame_fill or e264hip_frame_upload, with no wait between, sees that work's result.  All
 *   streams of a call, on both sides, belong to `dev` and share one lane, as for a submission (else EINVAL); a stream may appear more than once (the
 *   pass only reads).  The call waits for its own event, never for the device.
 * Lifetime: the call marks the lane as a fill does, so a slot freed while it runs stays parked behind it (e264hip_frame_free never hands memory
 *   back under a kernel); the caller drives the streams, as for a submission.
 * Errors: EINVAL (and nothing is queued, `out` is untouched) for a null pointer, n < 0, n > E264_BLOCKDIFF_MAX_BATCH, k outside 3..6, a slot out of
 *   range or not allocated, streams of two devices or two lanes, a view e264hip_view_check refuses for its own slot's size (either side), plane p of A
 *   and of B differing in width or height for any p, pitch or cap smaller than a pair's map, more than E264_BLOCKDIFF_MAX_BYTES in one call;
 *   e264hip_last_error() names the cause.  n == 0 returns 0.
 * e264hip_blockdiff_check (host only): e264hip_diff_check plus the range of k -- what the two calls ask of one pair; 0 or EINVAL with a text. */
typedef struct { uint32_t sad, sse; } E264BlockDiff;   /* 8 bytes: sum |a - b|, sum (a - b)^2 over the block's samples */
#define E264_BLOCKDIFF_VERSION 1
#define E264_BLOCKDIFF_MAX_BATCH 4096
#define E264_BLOCKDIFF_MAX_BYTES (1u << 28)   /* of one call: the sum of the pairs' maps, each rounded up to 16 */
size_t e264hip_blockdiff_bytes(const E264View *v, int log2_block, uint16_t dims[6]);
int  e264hip_blockdiff_check(const E264View *view_a, size_t slot_bytes_a, const E264View *view_b, size_t slot_bytes_b, int log2_block);
int  e264hip_frame_blockdiff(E264Stream *a, int slot_a, const E264View *view_a,
                             E264Stream *b, int slot_b, const E264View *view_b, int log2_block, void *out, size_t cap);
int  e264hip_blockdiff_batch(E264Device *dev,
                             E264Stream *const *streams_a, const int *slots_a, const E264View *views_a,
                             E264Stream *const *streams_b, const int *slots_b, const E264View *views_b,
                             int n, int log2_block, void *out, size_t pitch);

/* ---- what ONE decoded picture looks like, region by region: the per-block statistics map, computed on the device ---- */
/* The histogram has no positions, the block difference map needs a second picture, the preview is a mean without a second moment or gradients.
 * This map answers, block by block, for one picture where it lies: letterbox and pillarbox detection (rows or columns of flat blocks at one level),
 * regional black or frozen-logo detection, focus and blur meters (gradient energy), texture and activity masks for a downstream encoder's adaptive
 * quantisation, regions of interest for an inference stage, local mean and variance for auto-exposure -- without reading the picture back.  The
 * reference has no counterpart (include/edge264_blockstat.h's e264_blockstat_plane does the same arithmetic on an Edge264Frame's plane on the host).
 *
 * THE BLOCK STATISTICS MAP, version E264_BLOCKSTAT_VERSION.  k = log2_block in {3, 4, 5, 6}, b = 1 << k.  For plane p of a view, w x h samples s(y, x):
 *     bw = (w + b - 1) >> k          bh = (h + b - 1) >> k
 *     record (Y, X) covers the samples y in [b Y, min(b Y + b, h)), x in [b X, min(b X + b, w)):
 *         sum   = sum s                                sumsq = sum s^2                                  over the block's samples
 *         gh    = sum |s(y, x + 1) - s(y, x)|          over the block's samples (y, x) with x + 1 < w
 *         gv    = sum |s(y + 1, x) - s(y, x)|          over the block's samples (y, x) with y + 1 < h
 * A horizontal pair belongs to the block of its LEFT sample, also when x + 1 lies in the next block; a vertical pair to the block of its TOP
 * sample.  A pair that would leave the view does not exist.  Nothing is clamped or replicated: a block at the right or bottom edge simply has fewer
 * samples and pairs.  A picture's map is Y | Cb | Cr, each plane row-major bh x bw records, tight; every plane uses the same b, each over its own
 * (cropped) view, so the result stays 4:2:0.
 * Everything is exact: a block has at most 64 x 64 = 4096 samples, so sum, gh and gv are <= 4096 * 255 < 2^21 and sumsq <= 4096 * 255^2 < 2^29; the
 * accumulators are 32 bits and nothing wraps.
 * Per plane: the sum of `sum` over the map is sum n bin[n] of the histogram record of the same view and the sum of `sumsq` is sum n^2 bin[n]; the
 * block difference map of the picture against an all-zero picture of the same view has sad == sum and sse == sumsq, record for record; the sums of
 * gh and of gv over the map are the plane's total horizontal and vertical variation whatever k (a pair goes to one block only); and with n the
 * block's sample count, n sumsq - sum^2 >= 0 in 64 bits, zero <=> the block is flat.
 *
 * e264hip_blockstat_bytes (host only): the map's size, and in dims (may be NULL) bw, bh of Y, Cb, Cr; 0 for a null view, k outside 3..6 or a plane
 *   without samples.
 * e264hip_blockstat_batch: the map of views[i] of slot slots[i] of streams[i] at out + i * pitch; only its e264hip_blockstat_bytes bytes there are
 *   written, the rest of a pitch is left as it was.  e264hip_frame_blockstat is the batch of one with pitch = cap.  Both BLOCK until `out` (ordinary
 *   host memory) is filled.
 * Ordering: one kernel per call, whatever n, queued on the streams' compute lane behind everything queued there -- a map asked for right after
 *   e264hip_frame_submit, e264hip_submit_batch*, e264hip_frame_fill or e264hip_frame_upload, with no wait between, sees that work's result.  All
 *   streams of a call belong to `dev` and share one lane, as for a submission (else EINVAL); a stream may appear more than once (the pass only
 *   reads).  The call waits for its own event, never for the device.
 * Lifetime: the call marks the lane as a fill does, so a slot freed while it runs stays parked behind it (e264hip_frame_free never hands memory
 *   back under a kernel); the caller drives the streams, as for a submission.
 * Errors: EINVAL (and nothing is queued, `out` is untouched) for a null pointer, n < 0, n > E264_BLOCKSTAT_MAX_BATCH, k outside 3..6, a slot out of
 *   range or not allocated, streams of two devices or two lanes, a view e264hip_view_check refuses for that slot's size, pitch or cap smaller than a
 *   picture's map, more than E264_BLOCKSTAT_MAX_BYTES in one call; e264hip_last_error() names the cause.  n == 0 returns 0.
 * e264hip_blockstat_check (host only): e264hip_view_check plus the range of k -- what the two calls ask of one picture; 0 or EINVAL with a text. */
typedef struct { uint32_t sum, sumsq, gh, gv; } E264BlockStat;   /* 16 bytes: sum s, sum s^2, sum |right - s|, sum |below - s| over the block's samples */
#define E264_BLOCKSTAT_VERSION 1
#define E264_BLOCKSTAT_MAX_BATCH 4096
#define E264_BLOCKSTAT_MAX_BYTES (1u << 28)   /* of one call: the sum of the pictures' maps */
size_t e264hip_blockstat_bytes(const E264View *v, int log2_block, uint16_t dims[6]);
int  e264hip_blockstat_check(const E264View *view, size_t slot_bytes, int log2_block);
int  e264hip_frame_blockstat(E264Stream *s, int slot, const E264View *view, int log2_block, void *out, size_t cap);
int  e264hip_blockstat_batch(E264Device *dev, E264Stream *const *streams, const int *slots, const E264View *views,
                             int n, int log2_block, void *out, size_t pitch);

/* ---- batched, device-resident replay (multi-stream front end, benchmarking) ---- */
/* Uploads a packet once; the handle can then be replayed any number of times with the
 * command bytes already resident in HBM (bench.py's timed region). */
typedef struct E264Packet E264Packet;
int  e264hip_packet_upload(E264Device *dev, const void *packet, size_t bytes, E264Packet **out);
void e264hip_packet_free(E264Packet *p);
/* One launch over n (stream, packet) pairs: frame i of every stream.  All streams must be
 * distinct.  mode: E264_RUN_* bits. */
#define E264_RUN_RECON   1
#define E264_RUN_DEBLOCK 2
#define E264_RUN_ALL     3
int  e264hip_submit_batch(E264Device *dev, E264Stream *const *streams, E264Packet *const *packets, int n, int mode);
/* Host-only validation of a command packet (layout, per-macroblock offsets and indices): what every host-packet entry
 * point below runs before the packet may reach the device.  0 or EINVAL (e264hip_last_error() names the field). */
/* Build-time switches of the library, space separated ("" = the product build).  E264_ABL_* and E264_PHASE_* entries are timing
 * ablations whose samples are wrong by design: e264hip_device_open refuses such a build (ENOTSUP) unless E264_ALLOW_ABLATION=1 is in
 * the environment, and so do the loaders (edge264_amd/backend.py, the front end).  No counterpart in the reference (its variants are
 * all correct decoders, src/edge264.c:161-216). */
const char *e264hip_build_flags(void);
int  e264hip_packet_check(const void *packet, size_t bytes);
/* The WIRE form of a packet (version 5, or versions 6 and 7 for the second and third level of the fold; include/edge264_compact.h: fewer bytes over PCIe for pictures full of skipped / plain 16x16 macroblocks -- what the
 * stream itself spends a run length on, src/edge264_slice.c:1651-1849).  Every host-packet entry point (e264hip_frame_submit, e264hip_submit_batch_host /
 * _pinned, e264hip_packet_upload, e264hip_packet_check) takes either form; a wire packet is unfolded on the device by one more kernel in front of the four
 * (into a buffer of the stream's) and means exactly what its expansion means.  C callers use the inline functions of edge264_compact.h (the front end does);
 * these are the same functions for callers that do not compile C:
 *   e264hip_packet_compact_bound   capacity e264hip_packet_compact needs for this version-4 packet (0: not one)
 *   e264hip_packet_compact         version 4 (must pass e264hip_packet_check) -> version 5; returns the bytes written, 0 on error
 *   e264hip_packet_compact2_bound  the same for the fold at `level`
 *   e264hip_packet_compact2        the fold at `level`: 1 gives version 5 (the bytes of e264hip_packet_compact), 2 gives version 6, in which the inter
 *                                  macroblocks of one partition per list WITH residual are folded too (24 / 32 bytes instead of 40 / 48); any other level
 *                                  gives 0 and an error text.  Opt-in: nothing produces version 6 unless asked to
 *   e264hip_packet_fold_bound      the same for every level of the fold there is
 *   e264hip_packet_fold            levels 1 and 2 give the bytes of e264hip_packet_compact / _compact2; level 3 gives version 7, in which a run of equal plain
 *                                  entries in a row (a background of skipped macroblocks) travels as one entry and a bit per further macroblock; any other
 *                                  level gives 0 and an error text.  Opt-in as well; the expansion is that of the version-6 packet of the same picture
 *   e264hip_packet_expand          version 5, 6 or 7 -> the canonical version-4 packet; out == NULL: the size needed; 0 on error */
size_t e264hip_packet_compact_bound(const void *packet, size_t bytes);
size_t e264hip_packet_compact(const void *packet, size_t bytes, void *out, size_t cap);
size_t e264hip_packet_compact2_bound(const void *packet, size_t bytes, int level);
size_t e264hip_packet_compact2(const void *packet, size_t bytes, int level, void *out, size_t cap);
size_t e264hip_packet_fold_bound(const void *packet, size_t bytes, int level);
size_t e264hip_packet_fold(const void *packet, size_t bytes, int level, void *out, size_t cap);
size_t e264hip_packet_expand(const void *packet, size_t bytes, void *out, size_t cap);
/* Same for packets that still live in HOST memory (the finished frames of many decoders, src/edge264_headers.c:532-568,
 * one per stream): staged through each stream's pinned ring, copied and launched on the device queue without any
 * synchronisation; the host buffers may be reused on return.  This is what a multi-stream front end calls once per
 * round (edge264_amd/driver/e264_multi.cpp). */
int  e264hip_submit_batch_host(E264Device *dev, E264Stream *const *streams, const void *const *packets, const size_t *bytes, int n, int mode);
/* Same for packets assembled IN PLACE in page-locked memory (e264hip_host_alloc): no staging copy, the H2D transfer reads
 * the caller's buffer, which must stay untouched until the submission has retired (e264hip_event_record after the call, then
 * e264hip_event_query / e264hip_frame_wait / e264hip_device_sync).  This is the path of a front end whose
 * emitters write the finished frame straight into pinned memory (the reference's per-frame hand-over point,
 * src/edge264_headers.c:532-568).  flags: E264_SUBMIT_TRUSTED = these exact bytes have already passed
 * e264hip_packet_check (on the parser thread that produced them), the per-macroblock walk is not repeated here; the slots
 * the vetted header names (dst_slot, ref_slots -- packet_check verifies both against the records) are still checked
 * against the stream's allocations. */
#define E264_SUBMIT_TRUSTED 1
int  e264hip_submit_batch_pinned(E264Device *dev, E264Stream *const *streams, const void *const *packets, const size_t *bytes, int n, int mode, int flags);
void *e264hip_host_alloc(E264Device *dev, size_t bytes);
void e264hip_host_free(E264Device *dev, void *p);
/* Same, with the job table built once and kept in HBM: the launch itself moves no bytes
 * over PCIe (a persistent multi-stream front end re-submits frame i of every stream). */
typedef struct E264Batch E264Batch;
int  e264hip_batch_create(E264Device *dev, E264Stream *const *streams, E264Packet *const *packets, int n, E264Batch **out);
int  e264hip_batch_submit(E264Batch *b, int mode);
void e264hip_batch_free(E264Batch *b);

/* Timing on the queues the kernels run on (hipEvents; torch.cuda.Event would only see
 * torch's own stream).  Slots 0..15.  Recorded on lane 0 behind everything queued on the other lanes so far. */
int  e264hip_event_record(E264Device *dev, int idx);
int  e264hip_event_elapsed_ms(E264Device *dev, int idx_start, int idx_stop, float *ms);
/* 0 when everything queued before e264hip_event_record(dev, idx) has left the GPU, EBUSY while it has not; never blocks.
 * (How a front end that submits packets in place, e264hip_submit_batch_pinned, learns when their buffers may be reused.) */
int  e264hip_event_query(E264Device *dev, int idx);
/* Accumulated time of each of the four kernels of a submission (ms4[0] deblock-parameter kernel,
 * ms4[1] parallel MB kernel, ms4[2] intra wavefront, ms4[3] deblocking wavefront), measured with
 * events recorded on the queue between the launches (only when enabled). */
int  e264hip_kernel_timing(E264Device *dev, int enable);
int  e264hip_kernel_time_ms(E264Device *dev, double *ms4, int *launches);

/* Tunables; returns the previous value, -1 if unknown: "waves" / "intra_waves" (waves per frame workgroup of the two
 * wavefront kernels), "side_queue" (1 = the deblock-parameter kernel runs on a second HIP queue beside the parallel MB
 * kernel; its ms4[0] is then measured on that queue), "upload_queue" (default 1: the H2D copies of host batches run on
 * the device's upload queue beside the kernels of earlier batches; 0: on the lane itself, in order with them).
 * Timing ablations that skip work are separate builds of the library (csrc/Makefile `variant`, -DE264_ABL_*), never an
 * option of the product. */
int  e264hip_set_option(E264Device *dev, const char *name, int value);

/* Which kernel forms the launcher chose: pictures (jobs, not launches) that went through each form since the device was
 * opened or last reset, one uint64_t per slot in the order below.  Slot 0 holds the device's compute-unit count instead
 * (the size rules of the two-workgroup forms depend on it).  The intra slots are exclusive: a picture's intra pass is
 * counted once, under the split-off forms when it ran on the second queue.  dbkp_side1 / dbkp_side2 count the pictures
 * whose parameter kernel ran on the second queue (beside prediction / beside intra) on top of dbkp_small / dbkp_general.
 * Copies min(n, E264_LC_COUNT) slots; reset != 0 zeroes the counters after the copy.  Returns E264_LC_COUNT, or -1. */
#define E264_LC_NAMES "n_cus expand dbkp_small dbkp_general dbkp_side1 dbkp_side2 pred " \
	"intra4_bitmap intra8_bitmap intra16_bitmap intra4_nobitmap intra8_nobitmap intra16_nobitmap " \
	"intra_split intra_planes_split intra_planes_alone dbk_planes dbk2_6 dbk2_7 dbk2_8 dbk2_10 dbk2_12 dbk_2 dbk_4 dbk_7 dbk_8"
enum { E264_LC_N_CUS, E264_LC_EXPAND, E264_LC_DBKP_SMALL, E264_LC_DBKP_GENERAL, E264_LC_DBKP_SIDE1, E264_LC_DBKP_SIDE2, E264_LC_PRED,
	E264_LC_INTRA4_BITMAP, E264_LC_INTRA8_BITMAP, E264_LC_INTRA16_BITMAP, E264_LC_INTRA4_NOBITMAP, E264_LC_INTRA8_NOBITMAP, E264_LC_INTRA16_NOBITMAP,
	E264_LC_INTRA_SPLIT, E264_LC_INTRA_PLANES_SPLIT, E264_LC_INTRA_PLANES_ALONE, E264_LC_DBK_PLANES, E264_LC_DBK2_6, E264_LC_DBK2_7, E264_LC_DBK2_8,
	E264_LC_DBK2_10, E264_LC_DBK2_12, E264_LC_DBK_2, E264_LC_DBK_4, E264_LC_DBK_7, E264_LC_DBK_8, E264_LC_COUNT };
int  e264hip_launch_counts(E264Device *dev, uint64_t *out, int n, int reset);

#ifdef __cplusplus
}
#endif
#endif
