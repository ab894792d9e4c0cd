/* edge264_compact.h -- the WIRE form of a command packet (versions 5, 6 and 7): the same information as version 4 (edge264_cmd.h) in fewer bytes for the link.
 *
 * Why.  A packet crosses PCIe once and is then read by four kernels; with the copy inside the clock the back end runs at 0.9 of the link
 * (bench.py pcie_inclusive.link_frac), and most macroblocks of an encoder-made stream say "one vector per list, no residual" -- P_Skip, B_Skip / Direct with one
 * motion for the whole macroblock, plain 16x16 -- in 40 or 48 bytes: a 32-byte record of which 7 bytes carry information and an 8-byte motion record per list
 * (5 200 of the 8 160 macroblocks of an average picture of tests/golden/streams/nat1080_ipp30.264, 5 700 of cabac_hd1080_ibbp30.264).  The stream itself
 * spends a run length on them (mb_skip_run, src/edge264_slice.c:1651-1849 of the reference).
 *
 * What.  Version 5 keeps header, slice table, motion records and payload of version 4 and replaces the array of E264Mb by a table in which such a macroblock
 * is a 12-byte entry (one list) or a 20-byte entry (both lists); every other macroblock keeps its 32-byte record.  Two bitmaps (one bit per macroblock: compact
 * at all / both lists) and three numbers per macroblock row (byte offset of the row's first entry, compact and two-list macroblocks before the row) let ANY
 * macroblock's entry be found with two popcounts, so the table expands in parallel: on the DEVICE, by e264_expand_kernel (edge264_amd/csrc/e264_expand.h),
 * into the version-4 record array and motion section the four kernels read -- in a buffer of the stream's; the kernels change by where two pointers point -- and
 * on the HOST, by e264_expand_packet below, into a canonical version-4 packet (validation, oracle, tools).  Packets that stay in HBM (capture replay, benchmarks'
 * resident legs) are uploaded expanded.
 *
 *   [E264FrameHdr, version 5][E264SliceParams x n_slices]
 *   mbs_off ->  E264CompactHdr
 *               uint32_t row_off[height_mbs]                 byte offset of the row's first entry from the start of the entry area
 *               uint32_t row_cbase[height_mbs]               compact macroblocks in the rows before
 *               uint32_t row_bbase[height_mbs]               two-list compact macroblocks in the rows before
 *               uint32_t cbits[height_mbs][words_per_row]    bit x of row y: macroblock (x, y) is compact
 *               uint32_t bbits[height_mbs][words_per_row]    ... and predicts from both lists (a subset of cbits)
 *               (padding to 8)  entries in raster order: E264MbCompact (12 bytes), E264MbCompact + E264MbCompactL1 (20 bytes) or E264Mb (32 bytes; mot_off
 *                               counts in THIS packet's motion section)
 *   motion_off -> the motion records of the FULL inter macroblocks only      payload_off -> as in version 4
 *
 * Version 6 (level 2 of the fold; opt-in, version 5 stays what it is) also folds the inter macroblock of one partition per list WITH residual: the entry above
 * followed by a 12-byte tail E264MbCompactTail {coded, payload_off, nz_mask}, 24 bytes for one list and 32 for both (no gain in the table, but 16 bytes fewer
 * in the motion section), and its flags may carry E264_MBF_T8x8 and E264_MBF_LEV8.  The header grows to 24 bytes (n_resid) and a third bitmap follows bbits:
 *               uint32_t rbits[height_mbs][words_per_row]    ... and carries the residual tail (a subset of cbits)
 * An entry lies at row_off[y] + 32 x - 20 c + 8 b + 12 r (compact, two-list and residual macroblocks before it in the row: three popcounts); its motion
 * record's place depends on c and b alone, so the directory is the same.  The expansion is the same kind of thing: a canonical version-4 packet.
 *
 * Version 7 (level 3; opt-in as well, versions 5 and 6 stay what they are) is version 6 in which a RUN of equal plain entries -- a background of P_Skip /
 * B_Skip macroblocks: same flags, slot, index, slice, QPs and vector(s) -- travels as ONE entry.  The header grows to 32 bytes (E264CompactHdr3: n_repeat,
 * n_repeat_both) and a fourth bitmap follows rbits:
 *               uint32_t pbits[height_mbs][words_per_row]    ... and REPEATS: it has no bytes in the entry area and stands for the same entry as its SOURCE,
 *                                                             the nearest macroblock to its left in the row whose pbits bit is clear (in the word of x the
 *                                                             highest clear bit of pbits below x, else the highest clear bit of the nearest earlier word
 *                                                             that has one)
 * n_compact, n_both, row_cbase, row_bbase, cbits and bbits count a repeat like any compact macroblock, and it has its own 8- or 16-byte record in the expanded
 * motion section where the formula above puts it: the expansion of a version-7 packet is byte for byte that of the version-6 packet of the same picture.
 * The entry of a macroblock that does not repeat lies at row_off[y] + 32 x - 20 c + 8 b + 12 r - 12 p - 8 q (p, q: the repeats and the two-list repeats,
 * pbits & bbits, before it in the row: five popcounts).  Structure (e264_check_compact): pbits is a subset of cbits & ~rbits; bit 0 of every row is clear; the
 * macroblock to the left of a repeat is compact, has no tail and the same bbits bit.  By induction the source of a repeat is then a plain entry of the
 * repeat's own class in the repeat's own row, and every macroblock between the two is a repeat of it -- none of them has bytes, so the same sum taken at a
 * REPEAT points just behind its source's entry: 12 or 20 bytes back is the source, without a search (e264_expand_kernel finds it so; e264_expand_mb below
 * searches as the definition says, and the tests hold the one against the other).  The fold makes macroblock x > 0 a repeat iff its class is 1 or 2 without
 * the tail, its left neighbour (repeat or not) has the same class, and the 12 or 20 bytes it would write equal the left one's: never across a row start, a
 * full record or a tail.  Canonical form: a plain entry that equals a plain entry of its class directly to its left is refused (it would have been a repeat).
 *
 * Plain C99, no dependencies: the front end (C), the back end (C++) and, through the back end's exports, the Python tools share this one definition. */
#ifndef EDGE264_COMPACT_H
#define EDGE264_COMPACT_H
#include <stddef.h>
#include <string.h>
#include "edge264_cmd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define E264_VERSION_COMPACT 5u  /* level 1 of the fold */
#define E264_VERSION_COMPACT2 6u /* level 2: ... and the one-partition macroblocks with residual */
#define E264_VERSION_COMPACT3 7u /* level 3: ... and a run of equal plain entries as one entry */
/* level of the fold a packet of this version is in: 0 none (not a wire packet), 1, 2, 3 */
static inline int e264_wire_level(uint32_t version) { return version - E264_VERSION_COMPACT <= 2u ? (int)(version - E264_VERSION_COMPACT) + 1 : 0; }
/* mot_hdr of "one partition per list": the list's four quadrant bits + its uniform bit (edge264_cmd.h E264_MOT_*) */
#define E264_MOT_HDR_UNI0 0x10fu
#define E264_MOT_HDR_UNI1 0x2f0u
#define E264_MOT_HDR_UNI01 0x3ffu
#define E264_MBCF_LIST1 0x80u /* E264MbCompact.flags: the (single) list is list 1 */

typedef struct E264CompactHdr { /* at mbs_off of a wire packet: these 16 bytes in version 5, 24 in version 6 (E264CompactHdr2), 32 in version 7 (E264CompactHdr3) */
	uint32_t n_compact;      /* compact macroblocks, the two-list ones included */
	uint32_t n_both;         /* ... of which predict from both lists */
	uint32_t entries_bytes;  /* 32 * n_mbs - 20 * n_compact + 8 * n_both */
	uint32_t words_per_row;  /* (width_mbs + 31) / 32 */
} E264CompactHdr;
typedef struct E264CompactHdr2 { /* 24 bytes at mbs_off of a version-6 packet */
	uint32_t n_compact, n_both;
	uint32_t entries_bytes;  /* 32 * n_mbs - 20 * n_compact + 8 * n_both + 12 * n_resid */
	uint32_t words_per_row;
	uint32_t n_resid;        /* compact macroblocks that carry the residual tail */
	uint32_t zero;
} E264CompactHdr2;
typedef struct E264CompactHdr3 { /* 32 bytes at mbs_off of a version-7 packet */
	uint32_t n_compact, n_both; /* (repeats included) */
	uint32_t entries_bytes;  /* 32 * n_mbs - 20 * n_compact + 8 * n_both + 12 * n_resid - 12 * n_repeat - 8 * n_repeat_both */
	uint32_t words_per_row;
	uint32_t n_resid;
	uint32_t n_repeat;       /* compact macroblocks without bytes of their own: each stands for the entry of its source */
	uint32_t n_repeat_both;  /* ... of which predict from both lists */
	uint32_t zero;
} E264CompactHdr3;

typedef struct E264MbCompact { /* 12 bytes: an inter macroblock of ONE partition without residual */
	uint8_t flags;       /* E264Mb.flags: EDGE_LEFT, EDGE_TOP, DEBLOCK (a macroblock with any other flag keeps its full record) | E264_MBCF_LIST1 */
	uint8_t ref_slot;    /* refPic: DPB slot, 0..31 (of list 0 in a two-list entry) */
	uint8_t ref_idx;     /* refIdx, 0..31 */
	uint8_t slice;       /* E264Mb.slice (a macroblock of slice 256 or beyond keeps its full record) */
	uint8_t qp[3];
	uint8_t dbk_slice;   /* E264Mb.dbk_slice (< 256) */
	int16_t mv[2];
} E264MbCompact;
typedef struct E264MbCompactL1 { /* 8 bytes behind the E264MbCompact of a two-list macroblock: list 1, as its motion record has it */
	uint8_t ref_slot, ref_idx, zero[2];
	int16_t mv[2];
} E264MbCompactL1;
typedef struct E264MbCompactTail { /* 12 bytes at the end of a residual entry (version 6): the three fields of E264Mb the residual needs, as they are */
	uint32_t coded;
	uint32_t payload_off;
	uint16_t nz_mask;
	uint16_t zero;
} E264MbCompactTail;
/* E264Mb.flags an entry may carry (any other keeps the full record): without / with the tail */
#define E264_MBCF_PLAIN (E264_MBF_EDGE_LEFT | E264_MBF_EDGE_TOP | E264_MBF_DEBLOCK)
#define E264_MBCF_RESID (E264_MBCF_PLAIN | E264_MBF_T8x8 | E264_MBF_LEV8)
/* class of an entry: 0 the full record; else 1 (one list) or 2 (both lists), plus E264_CLS_RESID when the tail follows */
#define E264_CLS_RESID 4
E264_SIZE_CHECK(sizeof(E264CompactHdr) == 16, "E264CompactHdr");
E264_SIZE_CHECK(sizeof(E264CompactHdr2) == 24, "E264CompactHdr2");
E264_SIZE_CHECK(sizeof(E264CompactHdr3) == 32, "E264CompactHdr3");
E264_SIZE_CHECK(sizeof(E264MbCompactTail) == 12, "E264MbCompactTail");
E264_SIZE_CHECK(sizeof(E264MbCompact) == 12, "E264MbCompact");
E264_SIZE_CHECK(sizeof(E264MbCompactL1) == 8, "E264MbCompactL1");

static inline uint32_t e264_compact_entry_bytes(int cls) { return cls == 0 ? 32u : 4u + 8u * ((uint32_t)cls & 3u) + 3u * ((uint32_t)cls & E264_CLS_RESID); } /* 32 | 12, 20, 24, 32 */
static inline uint32_t e264_compact_hdr_bytes(int level) { return 8u + 8u * (uint32_t)level; } /* 16, 24, 32 */
static inline uint32_t e264_compact_table_bytes(uint32_t width_mbs, uint32_t height_mbs, int level)
{ /* header + directory + bitmaps (two, three at level 2, four at level 3), padded to 8: where the entry area starts (from mbs_off) */
	const uint32_t wpr = (width_mbs + 31u) >> 5;
	return (e264_compact_hdr_bytes(level) + 12u * height_mbs + (4u + 4u * (uint32_t)level) * height_mbs * wpr + 7u) & ~7u;
}

/* how can this version-4 record go at this level of the fold (level 3: as at level 2; whether it repeats is the fold's matter)?  The class of its entry (0: as it is).  rec: its motion record (NULL when the packet has no
 * motion section) */
static inline int e264_mb_compact_class(const E264Mb *m, const uint8_t *rec, int level)
{
	uint32_t d[2], r0, r1;
	if (m->kind != E264_MB_INTER || m->slice > 255 || m->dbk_slice > 255 || !rec)
		return 0;
	int resid = 0;
	if ((m->flags & ~E264_MBCF_PLAIN) || m->coded || m->nz_mask) { /* level 1: nothing but edge flags, no residual */
		if (level < 2 || (m->flags & ~E264_MBCF_RESID))
			return 0;
		resid = E264_CLS_RESID;
	}
	memcpy(d, m->modes, 8);
	memcpy(&r0, rec, 4);
	if (r0 & 0xffffe0e0u) /* slot and index below 32, the two spare bytes zero */
		return 0;
	if (d[1] == E264_MOT_HDR_UNI0 || d[1] == E264_MOT_HDR_UNI1)
		return 1 | resid;
	if (d[1] != E264_MOT_HDR_UNI01)
		return 0;
	memcpy(&r1, rec + 8, 4);
	return (r1 & 0xffffe0e0u) ? 0 : 2 | resid;
}

/* upper bound of what e264_compact_packet / e264_compact_sections write for a picture whose version-4 packet has this header */
static inline size_t e264_compact_bound(const void *v4, int level)
{
	const E264FrameHdr *h = (const E264FrameHdr *)v4;
	return (size_t)h->total_bytes + e264_compact_table_bytes(h->width_mbs, h->height_mbs, level) + 64;
}

/* The fold at `level` (1: version 5, 2: version 6, 3: version 7), from the SECTIONS of a version-4 packet wherever they lie (a front end folds straight out of its builder's
 * arrays; e264_compact_packet below folds a packet).  h: the version-4 header (magic, sizes, slices_off, mbs_off, n_slices, payload_bytes and the summary fields
 * are taken as they are; motion_off, payload_off, total_bytes, version are written anew).  mot: NULL when no macroblock is inter.  payload_len <=
 * h->payload_bytes bytes are copied, the rest is zeros.  The sections must be what e264hip_packet_check would accept.  Returns the wire size, 0 when `cap` is
 * too small or the level is none of them. */
static inline size_t e264_compact_sections(const E264FrameHdr *h, const void *slices, const E264Mb *mbs, const uint8_t *mot, const uint8_t *payload, size_t payload_len,
	int level, void *out, size_t cap)
{
	const uint32_t wm = h->width_mbs, hm = h->height_mbs, wpr = (wm + 31u) >> 5;
	const uint32_t tb = e264_compact_table_bytes(wm, hm, level);
	if (level < 1 || level > 3 || cap < (size_t)h->total_bytes + tb + 64)
		return 0;
	uint8_t *o = (uint8_t *)out;
	memcpy(o, h, sizeof(*h));
	memset(o + sizeof(*h), 0, h->slices_off - sizeof(*h));
	memcpy(o + h->slices_off, slices, sizeof(E264SliceParams) * (size_t)h->n_slices);
	const uint32_t send = h->slices_off + (uint32_t)sizeof(E264SliceParams) * h->n_slices;
	memset(o + send, 0, h->mbs_off - send + tb);
	E264FrameHdr *oh = (E264FrameHdr *)o;
	E264CompactHdr3 *ch = (E264CompactHdr3 *)(o + h->mbs_off); /* (level 1: its first 16 bytes, level 2: its first 24) */
	uint32_t *row_off = (uint32_t *)(o + h->mbs_off + e264_compact_hdr_bytes(level)), *row_cbase = row_off + hm, *row_bbase = row_cbase + hm, *cbits = row_bbase + hm,
		*bbits = cbits + hm * wpr, *rbits = bbits + hm * wpr, *pbits = rbits + hm * wpr; /* (rbits: from level 2, pbits: level 3) */
	uint8_t *ent = o + h->mbs_off + tb;
	uint32_t eoff = 0, nc = 0, nb = 0, nr = 0, np = 0, nq = 0, moff = 0;
	const E264Mb *m = mbs;
	for (uint32_t y = 0; y < hm; y++) {
		row_off[y] = eoff; row_cbase[y] = nc; row_bbase[y] = nb;
		int left_cls = 0;          /* class of the macroblock to the left (0 at a row start and behind a full record) ... */
		uint8_t left[20] = {0};    /* ... and the 12 or 20 bytes it wrote, or would have written were it not a repeat itself */
		for (uint32_t x = 0; x < wm; x++, m++) {
			if (m->kind != E264_MB_INTER) { memcpy(ent + eoff, m, 32); eoff += 32; left_cls = 0; continue; }
			uint32_t d[2];
			memcpy(d, m->modes, 8);
			const uint8_t *rec = mot ? mot + d[0] : NULL;
			const int cls = e264_mb_compact_class(m, rec, level);
			if (!cls) {
				memcpy(ent + eoff, m, 32);
				memcpy(ent + eoff + offsetof(E264Mb, modes), &moff, 4); /* mot_off in this packet's motion section */
				moff += e264_mot_record_bytes(d[1]);
				eoff += 32;
				left_cls = 0;
				continue;
			}
			uint8_t c[20]; /* E264MbCompact [+ E264MbCompactL1] */
			const uint32_t cb = (cls & 3) == 2 ? 20u : 12u, bit = 1u << (x & 31);
			c[0] = (uint8_t)(m->flags | (d[1] == E264_MOT_HDR_UNI1 ? E264_MBCF_LIST1 : 0)); c[1] = rec[0]; c[2] = rec[1]; c[3] = (uint8_t)m->slice;
			c[4] = m->qp[0]; c[5] = m->qp[1]; c[6] = m->qp[2]; c[7] = (uint8_t)m->dbk_slice;
			memcpy(c + 8, rec + 4, 4);
			if (cb == 20) memcpy(c + 12, rec + 8, 8);
			nc++;
			cbits[y * wpr + (x >> 5)] |= bit;
			if (cb == 20) { nb++; bbits[y * wpr + (x >> 5)] |= bit; }
			if (level == 3 && cls == left_cls && !(cls & E264_CLS_RESID) && !memcmp(c, left, cb)) { /* a repeat: no bytes (left_cls is 0 at x == 0) */
				np++; nq += cb == 20;
				pbits[y * wpr + (x >> 5)] |= bit;
				continue;
			}
			memcpy(ent + eoff, c, cb);
			if (level == 3) { memcpy(left, c, cb); left_cls = cls; }
			eoff += cb;
			if (cls & E264_CLS_RESID) {
				const E264MbCompactTail t = {m->coded, m->payload_off, m->nz_mask, 0};
				memcpy(ent + eoff, &t, 12);
				eoff += 12; nr++;
				rbits[y * wpr + (x >> 5)] |= bit;
			}
		}
	}
	ch->n_compact = nc; ch->n_both = nb; ch->entries_bytes = eoff; ch->words_per_row = wpr;
	if (level >= 2) ch->n_resid = nr;
	if (level == 3) { ch->n_repeat = np; ch->n_repeat_both = nq; }
	/* motion section: the records of the full inter macroblocks, in macroblock order (the bitmap says which are not) */
	uint32_t pos = (h->mbs_off + tb + eoff + 7u) & ~7u;
	memset(ent + eoff, 0, pos - (h->mbs_off + tb + eoff));
	oh->motion_off = moff ? pos : 0;
	if (moff) {
		m = mbs;
		for (uint32_t y = 0; y < hm; y++)
			for (uint32_t x = 0; x < wm; x++, m++) {
				if (m->kind != E264_MB_INTER || (cbits[y * wpr + (x >> 5)] >> (x & 31) & 1u)) continue;
				uint32_t d[2];
				memcpy(d, m->modes, 8);
				const uint32_t rb = e264_mot_record_bytes(d[1]);
				memcpy(o + pos, mot + d[0], rb);
				pos += rb;
			}
	}
	const uint32_t pad = ((pos + 7u) & ~7u) - pos;
	memset(o + pos, 0, pad);
	pos += pad;
	if (payload_len) memcpy(o + pos, payload, payload_len);
	memset(o + pos + payload_len, 0, h->payload_bytes - payload_len);
	oh->version = E264_VERSION_COMPACT + (uint32_t)level - 1u;
	oh->payload_off = pos;
	oh->total_bytes = pos + h->payload_bytes;
	return oh->total_bytes;
}

/* version 4 (already vetted: e264hip_packet_check, or the front end's own product) -> version 5 (level 1), 6 (level 2) or 7 (level 3).  Returns the wire size,
 * 0 when `cap` is too small, the input is not a version-4 packet or the level is none of them. */
static inline size_t e264_compact_packet(const void *v4, size_t bytes, int level, void *out, size_t cap)
{
	const uint8_t *p = (const uint8_t *)v4;
	const E264FrameHdr *h = (const E264FrameHdr *)v4;
	if (bytes < sizeof(*h) || h->magic != E264_MAGIC || h->version != E264_VERSION)
		return 0;
	return e264_compact_sections(h, p + h->slices_off, (const E264Mb *)(p + h->mbs_off), h->motion_off ? p + h->motion_off : NULL, p + h->payload_off, h->payload_bytes, level, out, cap);
}

/* Structure of a wire packet (version 5, 6 or 7, as its header says): everything an expansion (host or device) reads lies inside the packet and says what the
 * bitmaps say; a repeat of version 7 has a source (the rules in the header comment).  0 = sound. (What the records then MEAN is vetted on the expanded packet by the back end's per-macroblock walk, as for version 4.) */
static inline int e264_check_compact(const void *wire, size_t bytes)
{
	const uint8_t *p = (const uint8_t *)wire;
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	if (bytes < sizeof(*h) || h->magic != E264_MAGIC || !e264_wire_level(h->version) || h->total_bytes != bytes) return -1;
	const int level = e264_wire_level(h->version);
	const uint32_t wm = h->width_mbs, hm = h->height_mbs;
	if (wm == 0 || hm == 0 || hm > 1056) return -1;
	const uint64_t n = (uint64_t)wm * hm;
	const uint32_t wpr = (wm + 31u) >> 5, tb = e264_compact_table_bytes(wm, hm, level);
	if ((h->mbs_off & 7) || (uint64_t)h->slices_off + (uint64_t)h->n_slices * sizeof(E264SliceParams) > h->mbs_off || (uint64_t)h->mbs_off + tb > bytes) return -1;
	const E264CompactHdr3 *ch = (const E264CompactHdr3 *)(p + h->mbs_off); /* (version 5: its first 16 bytes, version 6: its first 24) */
	const uint32_t n_resid = level >= 2 ? ch->n_resid : 0, n_repeat = level == 3 ? ch->n_repeat : 0, n_repeat_both = level == 3 ? ch->n_repeat_both : 0;
	if (level == 2 && ((const E264CompactHdr2 *)ch)->zero) return -1;
	if (level == 3 && (ch->zero || n_repeat > ch->n_compact || n_repeat_both > n_repeat || n_repeat_both > ch->n_both)) return -1;
	if (n_resid > ch->n_compact) return -1;
	if (ch->words_per_row != wpr || ch->n_compact > n || ch->n_both > ch->n_compact
		|| ch->entries_bytes != 32ull * n - 20ull * ch->n_compact + 8ull * ch->n_both + 12ull * n_resid - 12ull * n_repeat - 8ull * n_repeat_both) return -1;
	const uint64_t end = (uint64_t)h->mbs_off + tb + ch->entries_bytes;
	if (end > bytes || (h->motion_off && (h->motion_off < end || h->motion_off > bytes)) || h->payload_off < end || (uint64_t)h->payload_off + h->payload_bytes > bytes) return -1;
	if ((h->motion_off && h->motion_off > h->payload_off) || ((h->slices_off | h->motion_off | h->payload_off) & 7)) return -1;
	const uint32_t *row_off = (const uint32_t *)(p + h->mbs_off + e264_compact_hdr_bytes(level)), *row_cbase = row_off + hm, *row_bbase = row_cbase + hm, *cbits = row_bbase + hm,
		*bbits = cbits + (size_t)hm * wpr, *rbits = bbits + (size_t)hm * wpr, *pbits = rbits + (size_t)hm * wpr;
	uint32_t eoff = 0, nc = 0, nb = 0, nr = 0, np = 0, nq = 0;
	for (uint32_t y = 0; y < hm; y++) {
		if (row_off[y] != eoff || row_cbase[y] != nc || row_bbase[y] != nb) return -1;
		uint32_t c = 0, b = 0, r = 0, pr = 0, q = 0, lc = 0, lb = 0, lr = 0; /* lc, lb, lr: the words to the left (none: zeros) */
		for (uint32_t w = 0; w < wpr; w++) {
			const uint32_t cw = cbits[y * wpr + w], bw = bbits[y * wpr + w], rw = level >= 2 ? rbits[y * wpr + w] : 0, pw = level == 3 ? pbits[y * wpr + w] : 0;
			if (w == wpr - 1 && (wm & 31) && (cw >> (wm & 31))) return -1; /* bits beyond the row */
			if ((bw | rw | pw) & ~cw) return -1;
			/* a repeat: no tail, and its left neighbour (bit 31 of the word before for bit 0; none for the row's first) is compact without a tail and of
			 * the same number of lists */
			const uint32_t left_c = cw << 1 | lc >> 31, left_b = bw << 1 | lb >> 31, left_r = rw << 1 | lr >> 31;
			if (pw & (rw | ~left_c | left_r | (bw ^ left_b))) return -1;
			lc = cw; lb = bw; lr = rw;
			c += (uint32_t)__builtin_popcount(cw); b += (uint32_t)__builtin_popcount(bw); r += (uint32_t)__builtin_popcount(rw);
			pr += (uint32_t)__builtin_popcount(pw); q += (uint32_t)__builtin_popcount(pw & bw);
		}
		nc += c; nb += b; nr += r; np += pr; nq += q; eoff += 32 * wm - 20 * c + 8 * b + 12 * r - 12 * pr - 8 * q;
	}
	if (nc != ch->n_compact || nb != ch->n_both || nr != n_resid || np != n_repeat || nq != n_repeat_both || eoff != ch->entries_bytes) return -1;
	/* the expansion is a version-4 packet: 32-bit offsets (and what the kernels add to them) */
	return ((uint64_t)h->mbs_off + 32 * n + (h->motion_off ? h->payload_off - h->motion_off : 0) + 8ull * nc + 8ull * nb + 8 + h->payload_bytes) >> 31 ? -1 : 0;
}

/* bytes of the motion section of the expansion: the wire's records, then 8 bytes per compact macroblock and list */
static inline size_t e264_expanded_motion_bytes(const void *wire)
{
	const uint8_t *p = (const uint8_t *)wire;
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	const E264CompactHdr *ch = (const E264CompactHdr *)(p + h->mbs_off);
	return (size_t)(h->motion_off ? h->payload_off - h->motion_off : 0) + (size_t)8 * ch->n_compact + (size_t)8 * ch->n_both; /* (all three multiples of 8) */
}
/* size of the canonical version-4 packet e264_expand_packet makes of this (structurally sound) wire packet, of any version: the residual tails of
 * version 6 go into records that are there anyway, and a repeat of version 7 is counted in n_compact / n_both like its source */
static inline size_t e264_expanded_bytes(const void *wire)
{
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	return (size_t)h->mbs_off + (size_t)32 * h->width_mbs * h->height_mbs + e264_expanded_motion_bytes(wire) + h->payload_bytes;
}
/* bytes of the DEVICE expansion (the stream's expansion buffer): the canonical packet's record array and motion section -- the same bytes e264_expand_packet
 * puts at mbs_off .. payload_off; the payload is read where the wire packet lies */
static inline size_t e264_expand_area_bytes(const void *wire)
{
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	return (size_t)32 * h->width_mbs * h->height_mbs + e264_expanded_motion_bytes(wire);
}

/* A compact entry of class `cls` (12, 20, 24 or 32 bytes) as what it stands for: the version-4 record, whose motion record lies at mot_off of the motion
 * section, and that motion record (rec; returns its 8 or 16 bytes). */
static inline uint32_t e264_compact_entry_expand(const uint8_t *e, int cls, uint32_t mot_off, E264Mb *out, uint8_t rec[16])
{
	const int both = (cls & 3) == 2;
	E264MbCompact k;
	memcpy(&k, e, 12);
	memset(out, 0, 32);
	out->kind = E264_MB_INTER; out->flags = (uint8_t)(k.flags & ~E264_MBCF_LIST1);
	out->qp[0] = k.qp[0]; out->qp[1] = k.qp[1]; out->qp[2] = k.qp[2];
	out->slice = k.slice; out->dbk_slice = k.dbk_slice;
	const uint32_t d[2] = {mot_off, both ? E264_MOT_HDR_UNI01 : (k.flags & E264_MBCF_LIST1) ? E264_MOT_HDR_UNI1 : E264_MOT_HDR_UNI0};
	memcpy(out->modes, d, 8);
	rec[0] = k.ref_slot; rec[1] = k.ref_idx; rec[2] = rec[3] = 0;
	memcpy(rec + 4, k.mv, 4);
	if (both) memcpy(rec + 8, e + 12, 8);
	if (cls & E264_CLS_RESID) {
		E264MbCompactTail t;
		memcpy(&t, e + (both ? 20 : 12), 12);
		out->coded = t.coded; out->payload_off = t.payload_off; out->nz_mask = t.nz_mask;
	}
	return both ? 16 : 8;
}

/* Is this entry of a version-6 or -7 packet the one the fold writes for the record it expands to?  Every spare bit zero (flag bits an entry may not carry,
 * slot and index below 32, E264MbCompactL1.zero, E264MbCompactTail.zero), a tail only where the plain entry could not say it and, in version 7, no plain
 * entry with bytes of its own that equals the entry of its left neighbour (`left`, of class left_cls; NULL in version 6, at a row start and for a repeat, which
 * IS its source's entry): then folding the expansion again gives the packet's own bytes.  1 = it is. */
static inline int e264_compact_entry_canonical(const uint8_t *e, int cls, const uint8_t *left, int left_cls)
{
	const int both = (cls & 3) == 2;
	uint32_t e0, l1 = 0;
	memcpy(&e0, e, 4);
	if (both) memcpy(&l1, e + 12, 4);
	if ((e0 & 0x00e0e000u) || (l1 & 0xffffe0e0u)) return 0;
	const uint32_t flags = e0 & 0x7fu;
	if (!(cls & E264_CLS_RESID)) return !(flags & ~(uint32_t)E264_MBCF_PLAIN) && !(left && left_cls == cls && !memcmp(e, left, both ? 20 : 12));
	E264MbCompactTail t;
	memcpy(&t, e + (both ? 20 : 12), 12);
	return !(flags & ~(uint32_t)E264_MBCF_RESID) && !t.zero && ((flags & ~(uint32_t)E264_MBCF_PLAIN) || t.coded || t.nz_mask);
}

/* The entries of a (structurally sound) wire packet one after the other, in raster order: the sequential form of e264_expand_mb's address arithmetic,
 * running counts instead of popcounts. */
typedef struct E264CompactCursor {
	const uint32_t *cbits, *bbits, *rbits, *pbits; /* bitmap words of the current row (rbits: NULL in version 5; pbits: NULL in versions 5 and 6) */
	const uint8_t *e;              /* the next entry */
	const uint8_t *src;            /* the last entry that had bytes of its own: what a repeat stands for */
	int repeat;                    /* the macroblock e264_cursor_next returned last is a repeat (*entry was its source's) */
	uint32_t x, wm, wpr;
	uint32_t nc, nb;               /* compact / two-list macroblocks before it: its motion record lies 8 * (nc + nb) bytes behind the first compact one's */
} E264CompactCursor;
static inline void e264_cursor_init(E264CompactCursor *c, const uint8_t *wire)
{
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	const int level = e264_wire_level(h->version);
	c->x = c->nc = c->nb = 0;
	c->wm = h->width_mbs; c->wpr = ((const E264CompactHdr *)(wire + h->mbs_off))->words_per_row;
	c->cbits = (const uint32_t *)(wire + h->mbs_off + e264_compact_hdr_bytes(level)) + 3 * (size_t)h->height_mbs;
	c->bbits = c->cbits + (size_t)h->height_mbs * c->wpr;
	c->rbits = level >= 2 ? c->bbits + (size_t)h->height_mbs * c->wpr : NULL;
	c->pbits = level == 3 ? c->rbits + (size_t)h->height_mbs * c->wpr : NULL;
	c->e = c->src = wire + h->mbs_off + e264_compact_table_bytes(h->width_mbs, h->height_mbs, level);
	c->repeat = 0;
}
/* the next macroblock's entry (*entry) and its class: 0 full record (32 bytes), 1 one list (12), 2 both lists (20), with E264_CLS_RESID 12 more; for a repeat
 * (c->repeat) the entry of its source, which is of the same class */
static inline int e264_cursor_next(E264CompactCursor *c, const uint8_t **entry)
{
	const uint32_t w = c->x >> 5, bit = c->x & 31;
	int cls = (int)(c->cbits[w] >> bit & 1u) + (int)(c->bbits[w] >> bit & 1u); /* (bbits is a subset of cbits) */
	if (c->rbits && (c->rbits[w] >> bit & 1u)) cls |= E264_CLS_RESID;           /* (so is rbits) */
	c->repeat = c->pbits && (c->pbits[w] >> bit & 1u);                          /* (and pbits, of cbits & ~rbits; never the row's first) */
	if (c->repeat)
		*entry = c->src;
	else {
		*entry = c->src = c->e;
		c->e += e264_compact_entry_bytes(cls);
	}
	c->nc += cls > 0; c->nb += (cls & 3) > 1;
	if (++c->x == c->wm) { c->x = 0; c->cbits += c->wpr; c->bbits += c->wpr; if (c->rbits) c->rbits += c->wpr; if (c->pbits) c->pbits += c->wpr; }
	return cls;
}

/* bits set in both of two bitmaps' words of a row in front of column x (one bitmap: give it twice) */
static inline uint32_t e264_bits_before(const uint32_t *row, const uint32_t *also, uint32_t x)
{
	uint32_t n = (uint32_t)__builtin_popcount(row[x >> 5] & also[x >> 5] & ((1u << (x & 31)) - 1u));
	for (uint32_t w = 0; w < (x >> 5); w++) n += (uint32_t)__builtin_popcount(row[w] & also[w]);
	return n;
}

/* the version-4 record of macroblock (x, y) of a wire packet and, for a compact one, its motion record (8 or 16 bytes, *rec_bytes; 0 for a full record).
 * synth_off: mot_off of the FIRST compact macroblock's motion record (they follow one another in macroblock order).  THE definition of the expansion: the
 * device kernel restates it.  A repeat of version 7 reads the entry of its source, searched for as the header comment defines it, and keeps its own place in
 * the motion section. */
static inline void e264_expand_mb(const uint8_t *wire, uint32_t x, uint32_t y, uint32_t synth_off, E264Mb *out, uint8_t rec[16], uint32_t *rec_bytes)
{
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	const E264CompactHdr *ch = (const E264CompactHdr *)(wire + h->mbs_off);
	const int level = e264_wire_level(h->version);
	const uint32_t hm = h->height_mbs, wpr = ch->words_per_row;
	const uint32_t *row_off = (const uint32_t *)(wire + h->mbs_off + e264_compact_hdr_bytes(level)), *row_cbase = row_off + hm, *row_bbase = row_cbase + hm, *cbits = row_bbase + hm,
		*bbits = cbits + hm * wpr, *rbits = level >= 2 ? bbits + hm * wpr : NULL, *pbits = level == 3 ? rbits + hm * wpr : NULL;
	const uint32_t cw = cbits[y * wpr + (x >> 5)], bw = bbits[y * wpr + (x >> 5)], rw = rbits ? rbits[y * wpr + (x >> 5)] : 0;
	const uint32_t *cr = cbits + y * wpr, *br = bbits + y * wpr, *rr = rbits ? rbits + y * wpr : NULL, *pr = pbits ? pbits + y * wpr : NULL;
	const uint32_t c = e264_bits_before(cr, cr, x), b = e264_bits_before(br, br, x);
	uint32_t sx = x; /* the macroblock whose entry this one reads: itself, or the source of a repeat */
	if (pr && (pr[x >> 5] >> (x & 31) & 1u)) {
		uint32_t w = x >> 5, clear = ~pr[w] & ((1u << (x & 31)) - 1u);
		while (!clear && w > 0) clear = ~pr[--w]; /* (bit 0 of the row is clear: ends in word 0 at the latest) */
		sx = clear ? 32u * w + 31u - (uint32_t)__builtin_clz(clear) : 0;
	}
	uint32_t eoff = row_off[y] + 32u * sx - 20u * e264_bits_before(cr, cr, sx) + 8u * e264_bits_before(br, br, sx);
	if (rr) eoff += 12u * e264_bits_before(rr, rr, sx);
	if (pr) eoff -= 12u * e264_bits_before(pr, pr, sx) + 8u * e264_bits_before(pr, br, sx);
	const uint8_t *e = wire + h->mbs_off + e264_compact_table_bytes(h->width_mbs, hm, level) + eoff;
	*rec_bytes = 0;
	if (!(cw >> (x & 31) & 1u)) { memcpy(out, e, 32); return; }
	const int cls = 1 + (int)(bw >> (x & 31) & 1u) + ((rw >> (x & 31) & 1u) ? E264_CLS_RESID : 0);
	*rec_bytes = e264_compact_entry_expand(e, cls, synth_off + 8u * (row_cbase[y] + c) + 8u * (row_bbase[y] + b), out, rec);
}

/* version 5, 6 or 7 (e264_check_compact has said 0) -> canonical version 4: [header][slices][E264Mb x n][motion: the wire's records, then the compact
 * macroblocks'][payload].  Returns the size, 0 when `cap` is too small. */
static inline size_t e264_expand_packet(const void *wire, size_t bytes, void *out, size_t cap)
{
	const uint8_t *p = (const uint8_t *)wire;
	const E264FrameHdr *h = (const E264FrameHdr *)wire;
	const size_t need = e264_expanded_bytes(wire);
	(void)bytes;
	if (cap < need) return 0;
	const E264CompactHdr *ch = (const E264CompactHdr *)(p + h->mbs_off);
	const uint32_t wm = h->width_mbs, hm = h->height_mbs, n = wm * hm;
	const uint32_t mot = h->motion_off ? h->payload_off - h->motion_off : 0; /* (the padding in front of the payload included: never addressed) */
	const uint32_t mtot = (uint32_t)e264_expanded_motion_bytes(wire);
	uint8_t *o = (uint8_t *)out;
	memcpy(o, p, h->mbs_off);
	E264FrameHdr *oh = (E264FrameHdr *)o;
	E264Mb *mbs = (E264Mb *)(o + h->mbs_off);
	const uint32_t mo = h->mbs_off + 32u * n;
	if (mot) memcpy(o + mo, p + h->motion_off, mot);
	for (uint32_t y = 0; y < hm; y++)
		for (uint32_t x = 0; x < wm; x++) {
			uint8_t rec[16];
			uint32_t rb;
			E264Mb *m = &mbs[y * wm + x];
			e264_expand_mb(p, x, y, mot, m, rec, &rb);
			if (rb) { uint32_t d[2]; memcpy(d, m->modes, 8); memcpy(o + mo + d[0], rec, rb); }
		}
	memcpy(o + mo + mtot, p + h->payload_off, h->payload_bytes);
	oh->version = E264_VERSION;
	oh->motion_off = (mot || ch->n_compact) ? mo : 0;
	oh->payload_off = mo + mtot;
	oh->total_bytes = mo + mtot + h->payload_bytes;
	return oh->total_bytes;
}

#ifdef __cplusplus
}
#endif
#endif
