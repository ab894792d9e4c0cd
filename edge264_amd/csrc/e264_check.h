// e264_check.h -- the gate in front of the GPU: what a command packet must satisfy before a kernel may read it.  Host code only (plain C++17, no HIP): it reads
// hostile bytes, so tools/sanitize/kernel_fuzz.py builds and runs it under AddressSanitizer.  e264_check.cpp also holds the entry points of include/edge264_hip.h
// that need no device (e264hip_packet_check, e264hip_packet_compact_bound, e264hip_packet_compact, e264hip_packet_compact2_bound, e264hip_packet_compact2, e264hip_packet_fold_bound, e264hip_packet_fold, e264hip_packet_expand, e264hip_view_check, e264hip_preview_bytes, e264hip_diff_check, e264hip_blockdiff_bytes, e264hip_blockdiff_check, e264hip_blockstat_bytes, e264hip_blockstat_check, e264hip_last_error).
#ifndef E264_CHECK_H
#define E264_CHECK_H
#include "../../include/edge264_hip.h"
#include "../../include/edge264_cmd.h"
#include "../../include/edge264_compact.h"

#define API extern "C" __attribute__((visibility("default")))

// The error text of the calling thread (e264hip_last_error): ONE buffer for the whole library.  The back end's pool workers copy it after a failed check.
extern thread_local char e264_err[256];
int e264_fail(int code, const char *what, const char *detail = nullptr); // writes "what[: detail]" to e264_err, returns code

// What the checks learn about a packet.  e264_check_header fills all of it (ref_mask from the header's summary, pred_work and has_l1 as "assume so");
// e264_check_records and e264_scan_trusted then set pred_work and has_l1 from the records.
struct E264PacketInfo {
	int dst_slot, width_mbs, height_mbs;
	size_t area;           // 0 for a version-4 packet; for a WIRE packet (versions 5 to 7, include/edge264_compact.h) the bytes its expansion on the device needs
	uint64_t frame_bytes;  // plane_size_Y + plane_size_C the kernels will touch in every slot the packet names
	uint32_t ref_mask;     // DPB slots its motion refers to
	bool pred_work;        // it holds inter or PCM macroblocks (else e264_pred_kernel has nothing to do for it)
	bool has_l1;           // some macroblock predicts from list 1 (else the parameter kernel's small form will do)
	int n_mbs() const { return width_mbs * height_mbs; }
};
// The allocations of a stream: slot pointers (null entry: not allocated) and slot sizes.  ptr == nullptr: no stream to hold the packet against.
struct E264SlotView { uint8_t *const *ptr; const size_t *bytes; };

// the header and the section layout (a wire packet: its whole structure, e264_check_compact)
int e264_check_header(const void *packet, size_t bytes, E264PacketInfo *info);
// everything a kernel will dereference through a packet that has passed e264_check_header (which filled `info`)
int e264_check_records(const void *packet, E264SlotView slots, E264PacketInfo *info);
// the destination and every reference slot of a vetted packet exist in `slots` and hold a picture of its size
int e264_check_slots(E264SlotView slots, const E264PacketInfo &info);
// pred_work / has_l1 of a packet its producer has vetted (E264_SUBMIT_TRUSTED), without the per-macroblock checks
void e264_scan_trusted(const void *packet, E264PacketInfo *info);
#endif
