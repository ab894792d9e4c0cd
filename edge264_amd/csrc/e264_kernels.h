// e264_kernels.h -- launch interface between the C-ABI back end and the gfx950 kernels.
#ifndef E264_KERNELS_H
#define E264_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "e264_plan.h"

// One job = one coded frame of one stream: its command packet (already in HBM) and the
// table of the stream's DPB slots (device pointers, E264_MAX_SLOTS entries, NULL if unallocated).
struct E264Job {
	const uint8_t *packet;
	uint8_t *const *dpb;
	uint8_t *dbk; // per-stream scratch, E264_SCRATCH_BYTES(macroblocks) (NULL: no deblocking, no intra bitmap -- host tests only, the back end always has one)
	uint8_t *expand; // per-stream expansion buffer of a WIRE packet (versions 5 to 7, include/edge264_compact.h: e264_expand_area_bytes), NULL for a version-4 packet
};
#define E264_DBK_BYTES 144 // sixteen 8-byte pieces in the layout of the deblocking kernel's lanes + 16 bytes for the whole macroblock (e264_dbkp.h)
// The scratch of a stream: the parameter records of n_mbs macroblocks, then the INTRA BITMAP of the picture being decoded: one uint16_t per
// (macroblock row, group of 16 macroblocks) = per row of a prediction tile, bit i = macroblock 16 g + i is Intra4x4 / 8x8 / 16x16 and this
// packet's to reconstruct.  Written by e264_pred_kernel (which reads every record anyway), read by e264_intra_kernel in the same submission
// to leave rows and 64-macroblock chunks without intra macroblocks alone (P / B pictures).  2 bytes per macroblock cover the worst shape (one column).
#define E264_SCRATCH_BYTES(n_mbs) ((size_t)(n_mbs) * (E264_DBK_BYTES + 2) + 64)
#define E264_BITMAP_OFF(n_mbs) ((size_t)(n_mbs) * E264_DBK_BYTES)

// What e264_launch_frames needs of a lane's second queue (the plan says whether anything runs there: the split-off intra pass or the parameter kernel):
// the queue, the events of its fork and join, and amarks: 2 events that bracket the kernel on it, recorded when marks != NULL.
struct E264Fork { hipStream_t aux; hipEvent_t forked, joined; hipEvent_t *amarks; };
// workgroups e264_pred_kernel needs for a picture of this size (its tile geometry is a build-time choice of the kernels)
extern "C" int e264_pred_tiles(int width_mbs, int height_mbs);
// build-time switches of the kernels ("" = product build; e264hip_build_flags hands it out)
extern "C" const char *e264_kernel_build_flags(void);
// Executes the plan (e264_plan.h: every choice of kernel is made there) for a job table of n jobs in the plan's order, on `stream`.
// max_mbs: largest macroblock count among the jobs; max_tiles: largest e264_pred_tiles() among the jobs.  marks: NULL or 5 events (boundaries of the 4 kernels).
extern "C" hipError_t e264_launch_frames(const E264Job *jobs, int n_jobs, int max_mbs, int max_tiles, const E264Plan &plan, hipStream_t stream, hipEvent_t *marks,
	const E264Fork &fork);

// e264_expand_kernel alone (a batch's wire packets, on the queue of its upload); E264Plan.expand runs it in front of the four instead
extern "C" hipError_t e264_launch_expand(const E264Job *jobs, int n_jobs, int max_mbs, hipStream_t stream);

// e264_digest_kernel (e264_digest.h, e264_digest.hip: a translation unit of its own).  One job = one picture to digest: the slot, its size -- the kernel reads no
// byte outside [base, base + slot_bytes) -- and where the samples lie in it (a view e264hip_view_check has accepted for slot_bytes).  base is 16-byte aligned
// (a device allocation).  chunks = e264_digest_chunks(view): the workgroups the picture gets.
struct E264DigestJob {
	const uint8_t *base;
	uint64_t slot_bytes;
	E264View view;
	uint32_t chunks;
};
extern "C" uint32_t e264_digest_chunks(const E264View *view);
// out[3 i + p] += the digest of plane p of job i: the caller clears out (3 n_jobs values) on `stream` in front.  max_chunks: the largest chunks among the jobs.
extern "C" hipError_t e264_launch_digest(const E264DigestJob *jobs, int n_jobs, uint32_t max_chunks, uint64_t *out, hipStream_t stream);

// e264_preview_kernel (e264_preview.h, e264_preview.hip: a translation unit of its own).  One job = one picture to reduce by 1 << k (k = 1, 2, 3): the slot and
// the view as for a digest job -- no byte outside [base, base + slot_bytes) is read -- and dst, where the picture's preview goes (device memory of
// e264hip_preview_bytes(view, k) bytes: every byte of it is written once, none outside it).  chunks = e264_preview_chunks(view, k).
struct E264PreviewJob {
	const uint8_t *base;
	uint64_t slot_bytes;
	E264View view;
	uint8_t *dst;
	uint32_t k;
	uint32_t chunks;
};
extern "C" uint32_t e264_preview_chunks(const E264View *view, int k);
extern "C" hipError_t e264_launch_preview(const E264PreviewJob *jobs, int n_jobs, uint32_t max_chunks, hipStream_t stream);

// e264_diff_kernel (e264_diff.h, e264_diff.hip: a translation unit of its own).  One job = one pair of pictures to compare: slot, size and view of each side as for
// a digest job -- no byte outside [base_a, base_a + slot_bytes_a) or [base_b, base_b + slot_bytes_b) is read -- where plane p of the two views has one width and
// height (e264hip_diff_check).  chunks = e264_diff_chunks(view_a).
struct E264DiffJob {
	const uint8_t *base_a;
	uint64_t slot_bytes_a;
	const uint8_t *base_b;
	uint64_t slot_bytes_b;
	E264View view_a, view_b;
	uint32_t chunks;
};
extern "C" uint32_t e264_diff_chunks(const E264View *view);
// out[i] accumulates the record of job i with `first` kept as ~first under a max: the caller clears out (n_jobs records) on `stream` in front and turns every
// `first` round (first = ~first) after the copy down.  max_chunks: the largest chunks among the jobs.
extern "C" hipError_t e264_launch_diff(const E264DiffJob *jobs, int n_jobs, uint32_t max_chunks, E264Diff *out, hipStream_t stream);

// e264_hist_kernel (e264_hist.h, e264_hist.hip: a translation unit of its own).  One job = one picture to count: slot, size and view as for a digest job -- no
// byte outside [base, base + slot_bytes) is read.  chunks = e264_hist_chunks(view).
struct E264HistJob {
	const uint8_t *base;
	uint64_t slot_bytes;
	E264View view;
	uint32_t chunks;
};
extern "C" uint32_t e264_hist_chunks(const E264View *view);
// out[i] accumulates the record of job i: the caller clears out (n_jobs records) on `stream` in front.  max_chunks: the largest chunks among the jobs.
extern "C" hipError_t e264_launch_hist(const E264HistJob *jobs, int n_jobs, uint32_t max_chunks, E264Hist *out, hipStream_t stream);

// e264_blockdiff_kernel (e264_blockdiff.h, e264_blockdiff.hip: a translation unit of its own).  One job = one pair of pictures to compare block by block
// (blocks of 1 << k, k = 3 .. 6): the two sides as for a diff job, and dst, where the pair's map goes (device memory of e264hip_blockdiff_bytes(view_a, k) bytes,
// 8-byte aligned: every record of it is written once, nothing outside it).  chunks = e264_blockdiff_chunks(view_a, k).
struct E264BlockDiffJob {
	const uint8_t *base_a;
	uint64_t slot_bytes_a;
	const uint8_t *base_b;
	uint64_t slot_bytes_b;
	E264View view_a, view_b;
	uint8_t *dst;
	uint32_t k;
	uint32_t chunks;
};
extern "C" uint32_t e264_blockdiff_chunks(const E264View *view, int k);
extern "C" hipError_t e264_launch_blockdiff(const E264BlockDiffJob *jobs, int n_jobs, uint32_t max_chunks, hipStream_t stream);

// e264_blockstat_kernel (e264_blockstat.h, e264_blockstat.hip: a translation unit of its own).  One job = one picture to describe block by block (blocks of
// 1 << k, k = 3 .. 6): slot, size and view as for a digest job -- no byte outside [base, base + slot_bytes) is read -- and dst, where the picture's map goes
// (device memory of e264hip_blockstat_bytes(view, k) bytes, 16-byte aligned: every record of it is written once, nothing outside it).
// chunks = e264_blockstat_chunks(view, k).
struct E264BlockStatJob {
	const uint8_t *base;
	uint64_t slot_bytes;
	E264View view;
	uint8_t *dst;
	uint32_t k;
	uint32_t chunks;
};
extern "C" uint32_t e264_blockstat_chunks(const E264View *view, int k);
extern "C" hipError_t e264_launch_blockstat(const E264BlockStatJob *jobs, int n_jobs, uint32_t max_chunks, hipStream_t stream);

#endif
