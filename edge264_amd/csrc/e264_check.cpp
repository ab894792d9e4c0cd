// e264_check.cpp -- validation of command packets (e264_check.h) and the entry points of include/edge264_hip.h that need no device.
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include "e264_check.h"
#include "../../include/edge264_preview.h"
#include "../../include/edge264_blockdiff.h"
#include "../../include/edge264_blockstat.h"

thread_local char e264_err[256];
int e264_fail(int code, const char *what, const char *detail)
{
	snprintf(e264_err, sizeof(e264_err), "%s%s%s", what, detail ? ": " : "", detail ? detail : "");
	return code;
}
#define fail e264_fail

API const char *e264hip_last_error(void) { return e264_err; }

int e264_check_header(const void *packet, size_t bytes, E264PacketInfo *info)
{
	const E264FrameHdr *h = (const E264FrameHdr *)packet;
	if (!packet || bytes < sizeof(*h) || h->magic != E264_MAGIC || (h->version != E264_VERSION && !e264_wire_level(h->version)) || h->total_bytes > bytes)
		return fail(EINVAL, "not a command packet");
	if (h->dst_slot < 0 || h->dst_slot >= E264_MAX_SLOTS) return fail(EINVAL, "dst_slot");
	if (e264_wire_level(h->version)) {
		if (e264_check_compact(packet, h->total_bytes)) return fail(EINVAL, "wire packet structure");
	} else {
		size_t n_mb = (size_t)h->width_mbs * h->height_mbs;
		size_t need = (size_t)h->mbs_off + n_mb * sizeof(E264Mb);
		if (h->motion_off && (h->motion_off < need || (need = (size_t)h->motion_off) > h->total_bytes)) return fail(EINVAL, "motion section");
		if (need > h->payload_off || (size_t)h->payload_off + h->payload_bytes > h->total_bytes) return fail(EINVAL, "packet layout");
	}
	*info = {h->dst_slot, h->width_mbs, h->height_mbs, e264_wire_level(h->version) ? e264_expand_area_bytes(packet) : 0,
		(uint64_t)h->plane_size_Y + h->plane_size_C, h->ref_slots, true, true};
	return 0;
}

// Everything a kernel will dereference through the packet, checked on the host before the packet may reach the
// device (a wild offset would be a GPU memory fault = process abort, not an error code): section layout, per-macroblock
// kind / slice index / payload bounds / intra modes, reference slots, and the header's summary fields (ref_slots,
// n_coded_mbs, n_inter_mbs) against the records -- the kernels' early exits and the trusted submission path rely on them.
// With the slots of a stream: a packet whose header claims a larger picture than the slot it writes or reads (SPS size
// change, stale capture, foreign packet) would make the kernels run past the allocation.
struct Walk {
	const E264FrameHdr *h;
	E264SlotView slots;
	uint64_t frame_need;
	uint32_t ref_mask = 0, n_coded = 0, n_inter = 0;
	bool pred_work = false, has_l1 = false;
};
// one macroblock record against its packet: m (the version-4 record), a / col (its address and column), mot / mot_bytes (the motion section its mot_off counts in)
static int check_mb(Walk &w, const E264Mb &m, int a, int col, const uint8_t *mot, uint32_t mot_bytes)
{
	const E264FrameHdr *h = w.h;
	if (m.kind > E264_MB_INTER) return fail(EINVAL, "macroblock kind");
	if (m.slice >= h->n_slices || m.dbk_slice >= h->n_slices) return fail(EINVAL, "macroblock slice index"); // every record: the parameter kernel reads the slice of absent macroblocks too
	if (m.kind == E264_MB_ABSENT) return 0;
	w.n_coded++;
	if (m.kind == E264_MB_INTER || m.kind == E264_MB_PCM) w.pred_work = true; // some macroblock is the prediction kernel's
	if ((m.flags & E264_MBF_T8x8) && (m.kind == E264_MB_I16x16 || m.kind == E264_MB_PCM)) return fail(EINVAL, "8x8 transform flag on an Intra16x16 / PCM macroblock");
	if ((m.payload_off & 7) || (uint64_t)m.payload_off + e264_mb_payload_bytes(&m) > h->payload_bytes) return fail(EINVAL, "macroblock payload");
	if ((m.flags & E264_MBF_EDGE_LEFT) && col == 0) return fail(EINVAL, "left edge flag on the first column");
	if ((m.flags & E264_MBF_EDGE_TOP) && a < h->width_mbs) return fail(EINVAL, "top edge flag on the first row");
	// internal intra modes (src/edge264_internal.h:564-634): the kernels index tables with them
	if (m.kind == E264_MB_I4x4) {
		uint64_t mm;
		memcpy(&mm, m.modes, 8); // 16 nibbles: above 13 <=> bits 1, 2 and 3 all set
		if ((mm >> 1) & (mm >> 2) & (mm >> 3) & 0x1111111111111111ull) return fail(EINVAL, "Intra4x4 mode");
	} else if (m.kind == E264_MB_I8x8) {
		for (int k = 0; k < 4; k++)
			if (m.modes[k] > 31) return fail(EINVAL, "Intra8x8 mode");
	} else if (m.kind == E264_MB_I16x16 && m.i16_mode > 6) return fail(EINVAL, "Intra16x16 mode");
	if (m.kind >= E264_MB_I4x4 && m.kind <= E264_MB_I16x16 && m.chroma_mode > 6) return fail(EINVAL, "intra chroma mode");
	if (m.kind == E264_MB_INTER) {
		w.n_inter++;
		if (!mot) return fail(EINVAL, "inter macroblock without motion section");
		uint32_t d[2];
		memcpy(d, m.modes, 8); // motion directory: record offset, shape
		if (E264_MOT_UNI(d[1], 1) || (d[1] >> 4 & 15u)) w.has_l1 = true; // predicts from list 1 (its uniform bit or one of its quadrant bits)
		if ((d[0] & 3) || d[1] >> 26 || (uint64_t)d[0] + e264_mot_record_bytes(d[1]) > mot_bytes) return fail(EINVAL, "macroblock motion record");
		// the record's reference dwords, where they lie (what e264_motion_expand would spread over 8 parts: the uniform form repeats
		// one dword, an unused quadrant of a partitioned list reads as -1, which is always admissible)
		const uint8_t *rec = mot + d[0];
		uint32_t n = 0;
		for (int l = 0; l < 2; l++) {
			const bool uni = E264_MOT_UNI(d[1], l);
			for (int q = 0; q < (uni ? 1 : 4); q++) {
				if (!uni && !E264_MOT_USED(d[1], l * 4 + q)) continue;
				const int rp = (int8_t)rec[n], ri = (int8_t)rec[n + 1];
				if (rp < 0 || rp >= E264_MAX_SLOTS) return fail(EINVAL, "reference slot"); // a part the directory announces predicts from a picture
				if (w.slots.ptr && !w.slots.ptr[rp]) return fail(EINVAL, "reference slot not allocated");
				if (w.slots.ptr && w.slots.bytes && w.frame_need > w.slots.bytes[rp]) return fail(EINVAL, "picture larger than a reference slot");
				w.ref_mask |= 1u << rp;
				if (ri < -1 || ri > 31) return fail(EINVAL, "reference index");
				n += uni ? 8 : 4 + 4 * e264_mot_nmv(E264_MOT_SUB(d[1], l * 4 + q));
			}
		}
	}
	return 0;
}

int e264_check_records(const void *packet, E264SlotView slots, E264PacketInfo *info)
{
	const E264FrameHdr *h = (const E264FrameHdr *)packet;
	const uint8_t *p = (const uint8_t *)packet;
	if (h->width_mbs == 0 || h->height_mbs == 0 || h->height_mbs > 1056) return fail(EINVAL, "frame size");
	if (h->n_slices == 0 || (size_t)h->slices_off + (size_t)h->n_slices * sizeof(E264SliceParams) > h->mbs_off) return fail(EINVAL, "slice section");
	if ((h->slices_off | h->mbs_off | h->motion_off | h->payload_off) & 7) return fail(EINVAL, "section alignment");
	if (h->stride_Y < (uint32_t)h->width_mbs * 16 || h->stride_C < (uint32_t)h->width_mbs * 16 || (h->stride_Y & 15) || (h->stride_C & 7))
		return fail(EINVAL, "strides");
	if ((uint64_t)h->plane_size_Y < (uint64_t)h->stride_Y * h->height_mbs * 16 || (uint64_t)h->plane_size_C < (uint64_t)h->stride_C * h->height_mbs * 8)
		return fail(EINVAL, "plane sizes");
	if (h->plane_size_Y & 15) return fail(EINVAL, "plane_size_Y alignment"); // chroma rows keep the 8 / 4-byte alignment of stride_C
	Walk w = {h, slots, info->frame_bytes};
	if (w.frame_need >= 1ull << 31) return fail(EINVAL, "picture of 2 GiB or more"); // (the kernels' slot offsets are 32-bit)
	if (slots.ptr && slots.bytes && slots.ptr[info->dst_slot] && w.frame_need > slots.bytes[info->dst_slot]) return fail(EINVAL, "picture larger than the destination slot");
	const uint8_t *mot = h->motion_off ? p + h->motion_off : nullptr; // compact motion records, up to payload_off
	const uint32_t mot_bytes = h->motion_off ? h->payload_off - h->motion_off : 0;
	if (e264_wire_level(h->version)) {
		// A wire packet (include/edge264_compact.h; e264_check_header has vetted its structure) means what its expansion means: every entry is held
		// against the same checks as the version-4 record e264_expand_kernel will make of it -- walked in place, entry by entry, without unfolding the packet.
		// Versions 6 and 7 are held to the canonical form as well (spare bits zero, a tail only where it says something, in version 7 no plain entry that equals
		// its left neighbour's and so should have been a repeat): folding the expansion again gives the packet's own bytes.  A repeat of version 7 is checked as
		// the record it expands to, at its own address: the entry is its source's.
		const int level = e264_wire_level(h->version);
		E264CompactCursor c;
		e264_cursor_init(&c, p);
		const uint8_t *left = nullptr; // version 7: the entry of the macroblock to the left in the row, of class left_cls
		for (int a = 0, r, n_mbs = info->n_mbs(), col = 0, left_cls = 0; a < n_mbs; a++, col = col + 1 == h->width_mbs ? 0 : col + 1) {
			const uint8_t *e;
			const int cls = e264_cursor_next(&c, &e);
			E264Mb m;
			uint8_t rec[16];
			if (!cls) { memcpy(&m, e, 32); r = check_mb(w, m, a, col, mot, mot_bytes); }
			else if (level >= 2 && !c.repeat && !e264_compact_entry_canonical(e, cls, col ? left : nullptr, left_cls)) r = fail(EINVAL, "wire entry not in canonical form");
			else r = check_mb(w, m, a, col, rec, e264_compact_entry_expand(e, cls, 0, &m, rec));
			if (r) return r;
			if (level == 3) { left = e; left_cls = cls; }
		}
	} else {
		const E264Mb *mbs = (const E264Mb *)(p + h->mbs_off);
		for (int a = 0, r, n_mbs = info->n_mbs(), col = 0; a < n_mbs; a++, col = col + 1 == h->width_mbs ? 0 : col + 1)
			if ((r = check_mb(w, mbs[a], a, col, mot, mot_bytes))) return r;
	}
	if (h->n_coded_mbs != w.n_coded || h->n_inter_mbs != w.n_inter) return fail(EINVAL, "header macroblock counts differ from the records");
	if (h->ref_slots != w.ref_mask) return fail(EINVAL, "header ref_slots differs from the motion records");
	info->pred_work = w.pred_work;
	info->has_l1 = w.has_l1;
	return 0;
}

// (after e264_check_records, or for a packet whose producer has run it: the header summarises the records)
int e264_check_slots(E264SlotView slots, const E264PacketInfo &info)
{
	if (!slots.ptr[info.dst_slot]) return fail(EINVAL, "destination slot not allocated");
	if (info.frame_bytes > slots.bytes[info.dst_slot]) return fail(EINVAL, "picture larger than the destination slot");
	for (int sl = 0; sl < E264_MAX_SLOTS; sl++)
		if (info.ref_mask >> sl & 1) {
			if (!slots.ptr[sl]) return fail(EINVAL, "reference slot not allocated");
			if (info.frame_bytes > slots.bytes[sl]) return fail(EINVAL, "picture larger than a reference slot");
		}
	return 0;
}

// What the launcher wants to know about a packet its producer has vetted (E264_SUBMIT_TRUSTED: the header summarises the records, the records are sound) without the
// per-macroblock walk: does any macroblock have work for the prediction kernel (inter, I_PCM), does any predict from list 1 (else the parameter kernel's small form
// will do)?  One byte / one dword per record: ~10 us per 1080p packet, on the thread that gathers it.
static bool record_has_l1(const uint8_t *rec) // a full record: an inter macroblock whose motion directory names list 1
{
	uint32_t mh;
	if (rec[0] != E264_MB_INTER) return false;
	memcpy(&mh, rec + offsetof(E264Mb, modes) + 4, 4);
	return E264_MOT_UNI(mh, 1) || (mh >> 4 & 15u);
}
void e264_scan_trusted(const void *packet, E264PacketInfo *info)
{
	const E264FrameHdr *h = (const E264FrameHdr *)packet;
	const uint8_t *p = (const uint8_t *)packet;
	const int n_mbs = info->n_mbs();
	bool l1 = false;
	if (h->version == E264_VERSION) {
		const uint8_t *rec = p + h->mbs_off;
		bool pw = h->n_inter_mbs != 0;
		for (int a = 0; a < n_mbs && !(pw && l1); a++, rec += sizeof(E264Mb)) {
			if (rec[0] == E264_MB_PCM) pw = true;
			else if (record_has_l1(rec)) l1 = true;
			if (!h->n_inter_mbs && pw) break; // (no inter macroblock: nothing more to learn)
		}
		info->pred_work = pw; info->has_l1 = l1;
	} else { // (folded: it has inter macroblocks; its structure was checked by e264_check_header)
		if (((const E264CompactHdr *)(p + h->mbs_off))->n_both) return; // (pred_work and has_l1 stay true)
		E264CompactCursor c;
		e264_cursor_init(&c, p);
		for (int a = 0; a < n_mbs && !l1; a++) {
			const uint8_t *e;
			l1 = e264_cursor_next(&c, &e) ? e[0] & E264_MBCF_LIST1 : record_has_l1(e);
		}
		info->has_l1 = l1;
	}
}

// host-only entry point of the checks (tests, front ends that want to vet a capture file)
API int e264hip_packet_check(const void *packet, size_t bytes)
{
	E264PacketInfo info;
	int r = e264_check_header(packet, bytes, &info);
	return r ? r : e264_check_records(packet, {nullptr, nullptr}, &info);
}

// Where a picture's samples lie in a slot of slot_bytes (E264View, include/edge264_hip.h): what the digest kernel may read.  Every sum in 64 bits:
// offset and stride are 32-bit and height 16-bit, so offset + (height - 1) * stride + width stays below 2^49 and cannot wrap.
API int e264hip_view_check(const E264View *v, size_t slot_bytes)
{
	static const char *const names[3] = {"Y", "Cb", "Cr"};
	if (!v) return fail(EINVAL, "view_check: null view");
	for (int p = 0; p < 3; p++) {
		const E264PlaneView &pl = v->plane[p];
		if (pl.width < 1 || pl.height < 1) return fail(EINVAL, "view_check: a plane without samples", names[p]);
		if (pl.stride < pl.width) return fail(EINVAL, "view_check: stride below width", names[p]);
		const uint64_t end = (uint64_t)pl.offset + (uint64_t)(pl.height - 1u) * pl.stride + pl.width;
		if (end > (uint64_t)slot_bytes) return fail(EINVAL, "view_check: the plane leaves the slot", names[p]);
	}
	return 0;
}

// The size of a view's preview at reduction k (include/edge264_hip.h: Y | Cb | Cr, each plane tight) and its planes' sizes; 0 for what has none.
API size_t e264hip_preview_bytes(const E264View *v, int log2_factor, uint16_t dims[6])
{
	size_t bytes = 0;
	unsigned d[6];
	if (!v) return 0;
	for (int p = 0; p < 3; p++) {
		if (!e264_preview_dims(v->plane[p].width, v->plane[p].height, log2_factor, &d[2 * p], &d[2 * p + 1])) return 0;
		bytes += (size_t)d[2 * p] * d[2 * p + 1];
	}
	if (dims)
		for (int i = 0; i < 6; i++) dims[i] = (uint16_t)d[i];
	return bytes;
}

// What a difference record (include/edge264_hip.h) asks of one pair: each view sound for its own slot, and plane p of the two of one size -- the diff kernel
// walks both pictures with A's widths and heights.
API int e264hip_diff_check(const E264View *a, size_t slot_bytes_a, const E264View *b, size_t slot_bytes_b)
{
	static const char *const names[3] = {"Y", "Cb", "Cr"};
	int r;
	if (!a || !b) return fail(EINVAL, "diff_check: null view");
	if ((r = e264hip_view_check(a, slot_bytes_a)) || (r = e264hip_view_check(b, slot_bytes_b))) return r;
	for (int p = 0; p < 3; p++)
		if (a->plane[p].width != b->plane[p].width || a->plane[p].height != b->plane[p].height)
			return fail(EINVAL, "diff_check: the two views' planes differ in size", names[p]);
	return 0;
}

// The size of a pair's block difference map at block size 1 << k (include/edge264_hip.h: Y | Cb | Cr, each plane bh x bw records, tight) and its planes' sizes;
// 0 for what has none.  (At most 3 * 8192 * 8192 records of 8 bytes: below 2^31.)
API size_t e264hip_blockdiff_bytes(const E264View *v, int log2_block, uint16_t dims[6])
{
	size_t bytes = 0;
	unsigned d[6];
	if (!v) return 0;
	for (int p = 0; p < 3; p++) {
		if (!e264_blockdiff_dims(v->plane[p].width, v->plane[p].height, log2_block, &d[2 * p], &d[2 * p + 1])) return 0;
		bytes += (size_t)d[2 * p] * d[2 * p + 1] * sizeof(E264BlockDiff);
	}
	if (dims)
		for (int i = 0; i < 6; i++) dims[i] = (uint16_t)d[i];
	return bytes;
}

// What a block difference map asks of one pair: what a difference record asks, and a block size the kernel has
API int e264hip_blockdiff_check(const E264View *a, size_t slot_bytes_a, const E264View *b, size_t slot_bytes_b, int log2_block)
{
	if (log2_block < 3 || log2_block > 6) return fail(EINVAL, "blockdiff_check: log2_block is none of 3, 4, 5, 6");
	return e264hip_diff_check(a, slot_bytes_a, b, slot_bytes_b);
}

// The size of a picture's block statistics map at block size 1 << k (include/edge264_hip.h: Y | Cb | Cr, each plane bh x bw records, tight) and its planes'
// sizes; 0 for what has none.  (At most 3 * 8192 * 8192 records of 16 bytes: below 2^32.)
API size_t e264hip_blockstat_bytes(const E264View *v, int log2_block, uint16_t dims[6])
{
	size_t bytes = 0;
	unsigned d[6];
	if (!v) return 0;
	for (int p = 0; p < 3; p++) {
		if (!e264_blockstat_dims(v->plane[p].width, v->plane[p].height, log2_block, &d[2 * p], &d[2 * p + 1])) return 0;
		bytes += (size_t)d[2 * p] * d[2 * p + 1] * sizeof(E264BlockStat);
	}
	if (dims)
		for (int i = 0; i < 6; i++) dims[i] = (uint16_t)d[i];
	return bytes;
}

// What a block statistics map asks of one picture: what every pass asks of a view, and a block size the kernel has
API int e264hip_blockstat_check(const E264View *view, size_t slot_bytes, int log2_block)
{
	if (log2_block < 3 || log2_block > 6) return fail(EINVAL, "blockstat_check: log2_block is none of 3, 4, 5, 6");
	return e264hip_view_check(view, slot_bytes);
}

// The wire form (include/edge264_compact.h) for callers that do not compile C: the Python tools, a binding in another language.
// e264hip_packet_fold takes every level; _compact2 keeps what it took when it was written (1 and 2), _compact is level 1.
API size_t e264hip_packet_fold_bound(const void *packet, size_t bytes, int level)
{
	const E264FrameHdr *h = (const E264FrameHdr *)packet;
	if (level < 1 || level > 3) { fail(EINVAL, "packet_fold: level is none of 1, 2, 3"); return 0; }
	return (packet && bytes >= sizeof(*h) && h->magic == E264_MAGIC && h->version == E264_VERSION) ? e264_compact_bound(packet, level) : 0;
}
// version 4 -> version 5 (level 1), 6 (level 2) or 7 (level 3); the input must pass e264hip_packet_check (checked here).  Returns the size written, 0 on error (e264hip_last_error).
API size_t e264hip_packet_fold(const void *packet, size_t bytes, int level, void *out, size_t cap)
{
	const E264FrameHdr *h = (const E264FrameHdr *)packet;
	if (level < 1 || level > 3) { fail(EINVAL, "packet_fold: level is none of 1, 2, 3"); return 0; }
	if (!packet || !out || bytes < sizeof(*h) || h->version != E264_VERSION || e264hip_packet_check(packet, bytes)) { fail(EINVAL, "packet_fold: not a sound version-4 packet"); return 0; }
	const size_t r = e264_compact_packet(packet, h->total_bytes, level, out, cap);
	if (!r) fail(EINVAL, "packet_fold: output buffer too small");
	return r;
}
API size_t e264hip_packet_compact2_bound(const void *packet, size_t bytes, int level)
{
	if (level != 1 && level != 2) { fail(EINVAL, "packet_compact: level is neither 1 nor 2"); return 0; }
	return e264hip_packet_fold_bound(packet, bytes, level);
}
API size_t e264hip_packet_compact_bound(const void *packet, size_t bytes) { return e264hip_packet_fold_bound(packet, bytes, 1); }
API size_t e264hip_packet_compact2(const void *packet, size_t bytes, int level, void *out, size_t cap)
{
	if (level != 1 && level != 2) { fail(EINVAL, "packet_compact: level is neither 1 nor 2"); return 0; }
	return e264hip_packet_fold(packet, bytes, level, out, cap);
}
API size_t e264hip_packet_compact(const void *packet, size_t bytes, void *out, size_t cap) { return e264hip_packet_fold(packet, bytes, 1, out, cap); }
// version 5, 6 or 7 -> the canonical version-4 packet.  out == NULL: the size needed.  0 on error.
API size_t e264hip_packet_expand(const void *packet, size_t bytes, void *out, size_t cap)
{
	E264PacketInfo info;
	const E264FrameHdr *h = (const E264FrameHdr *)packet;
	if (e264_check_header(packet, bytes, &info) || !e264_wire_level(h->version)) { fail(EINVAL, "packet_expand: not a sound wire packet"); return 0; }
	if (!out) return e264_expanded_bytes(packet);
	const size_t r = e264_expand_packet(packet, h->total_bytes, out, cap);
	if (!r) fail(EINVAL, "packet_expand: output buffer too small");
	return r;
}
