// e264_expand.h -- e264_expand_kernel: a WIRE packet (version 5, 6 or 7, include/edge264_compact.h) back into the record array and motion section the four
// kernels read, in the stream's expansion buffer (E264Job.expand):  [E264Mb x n_mbs][the wire's motion records][one 8-byte record per compact macroblock and list].
// One thread per macroblock restates e264_expand_mb (THE definition; tests/test_compact.py, test_compact2.py and test_compact3.py hold this source, compiled
// for the host, against it byte for byte: two popcounts find an entry of version 5, three one of version 6, whose residual entries end in {coded, payload_off,
// nz_mask}, five one of version 7, in which a REPEAT has no bytes and reads the entry of its source.  No search for the source: the macroblocks between the two
// are repeats without bytes as well, so the five-popcount sum taken at a repeat points just behind its source's entry -- 12 or 20 bytes back, a plain entry of
// the repeat's own class by the rules e264_check_compact holds every packet to, inside the entry area whatever else the bytes say),
// then the threads of the grid copy the wire's motion section dword by dword.  HBM-bound and small: 0.3 MB written per 1080p picture.
#ifndef E264_EXPAND_H
#define E264_EXPAND_H
#include "e264_dev.h"
#include "../../include/edge264_compact.h"

namespace {

#define XP_NT 256

// thread `t` of `nt` (the whole grid row of this job)
E264_DEV void expand_thread(const E264Job &job, const uint32_t t, const uint32_t nt)
{
	const uint8_t *pkt = job.packet;
	chdr_t h = (chdr_t)pkt;
	if (h->magic != E264_MAGIC || h->version - E264_VERSION_COMPACT > 2u || !job.expand)
		return;
	const bool v6 = h->version >= E264_VERSION_COMPACT2; // header of 24 bytes instead of 16, a third bitmap
	const bool v7 = h->version == E264_VERSION_COMPACT3; // ... of 32 bytes, a fourth bitmap
	const uint32_t wm = h->width_mbs, hm = h->height_mbs, n = wm * hm;
	const gu32 *tab = (const gu32 *)(pkt + h->mbs_off);
	const uint32_t wpr = tab[3];
	const gu32 *row_off = tab + (v7 ? 8 : v6 ? 6 : 4), *row_cbase = row_off + hm, *row_bbase = row_cbase + hm, *cbits = row_bbase + hm, *bbits = cbits + hm * wpr;
	const gu32 *rbits = v6 ? bbits + hm * wpr : cbits; // (version 5: never read)
	const gu32 *pbits = v7 ? rbits + hm * wpr : cbits; // (versions 5 and 6: never read)
	const uint8_t *ent = pkt + h->mbs_off + (((v7 ? 32u : v6 ? 24u : 16u) + 12u * hm + (v7 ? 16u : v6 ? 12u : 8u) * hm * wpr + 7u) & ~7u); // e264_compact_table_bytes
	const uint32_t mot = h->motion_off ? h->payload_off - h->motion_off : 0;
	gu32 *out = (gu32 *)job.expand;
	gu32 *omot = out + 8 * n;
	for (uint32_t a = t; a < n; a += nt) {
		const uint32_t y = a / wm, x = a - y * wm;
		uint32_t c = 0, b = 0, r = 0, p = 0, q = 0; // compact, two-list, residual, repeated and two-list repeated macroblocks before x in the row
		for (uint32_t w = 0; w < (x >> 5); w++) {
			const uint32_t bw = bbits[y * wpr + w];
			c += (uint32_t)__builtin_popcount(cbits[y * wpr + w]); b += (uint32_t)__builtin_popcount(bw);
			if (v6) r += (uint32_t)__builtin_popcount(rbits[y * wpr + w]);
			if (v7) { const uint32_t pw = pbits[y * wpr + w]; p += (uint32_t)__builtin_popcount(pw); q += (uint32_t)__builtin_popcount(pw & bw); }
		}
		const uint32_t cw = cbits[y * wpr + (x >> 5)], bw = bbits[y * wpr + (x >> 5)], rw = v6 ? rbits[y * wpr + (x >> 5)] : 0u, pw = v7 ? pbits[y * wpr + (x >> 5)] : 0u,
			below = (1u << (x & 31)) - 1u;
		c += (uint32_t)__builtin_popcount(cw & below); b += (uint32_t)__builtin_popcount(bw & below); r += (uint32_t)__builtin_popcount(rw & below);
		p += (uint32_t)__builtin_popcount(pw & below); q += (uint32_t)__builtin_popcount(pw & bw & below);
		uint32_t eoff = row_off[y] + 32u * x - 20u * c + 8u * b + 12u * r - 12u * p - 8u * q; // entries are 12, 20, 24 or 32 bytes: dword-aligned
		if (pw >> (x & 31) & 1u) eoff -= (bw >> (x & 31) & 1u) ? 20u : 12u; // a repeat: the entry in front of this place is its source's (see above)
		const gu32 *e = (const gu32 *)(ent + eoff);
		gv4u *o = (gv4u *)(out + 8 * a); // two 16-byte stores per record
		if (!(cw >> (x & 31) & 1u)) {
			const v4u lo = ((const gv4u *)e)[0], hi = ((const gv4u *)e)[1];
			o[0] = lo; o[1] = hi;
			continue;
		}
		// E264MbCompact {flags, ref_slot, ref_idx, slice | qp[3], dbk_slice | mv[2]} [E264MbCompactL1 {ref_slot, ref_idx, 0, 0 | mv[2]}]
		// [E264MbCompactTail {coded | payload_off | nz_mask, 0}] ->
		// E264Mb {kind, flags, qp0, qp1 | qp2, chroma_mode, i16_mode, - | nz_mask, slice | coded | payload_off | mot_off | mot_hdr | dbk_slice, -}
		const bool both = bw >> (x & 31) & 1u;
		const uint32_t e0 = e[0], e1 = e[1], e2 = e[2];
		uint32_t coded = 0, poff = 0, nz = 0;
		if (rw >> (x & 31) & 1u) { // the tail, as three dwords behind the list(s)
			const gu32 *tl = e + (both ? 5 : 3);
			coded = tl[0]; poff = tl[1]; nz = tl[2] & 0xffffu;
		}
		const uint32_t k = 2 * (row_cbase[y] + c) + 2 * (row_bbase[y] + b); // dwords of compact motion records before this one
		o[0] = (v4u){E264_MB_INTER | (e0 & 0x7fu) << 8 | (e1 & 0xffffu) << 16, e1 >> 16 & 255u, nz | (e0 >> 24) << 16, coded};
		o[1] = (v4u){poff, mot + 4u * k, both ? E264_MOT_HDR_UNI01 : (e0 & E264_MBCF_LIST1) ? E264_MOT_HDR_UNI1 : E264_MOT_HDR_UNI0, e1 >> 24};
		gv2u *rec = (gv2u *)(omot + (mot >> 2) + k);
		rec[0] = (v2u){e0 >> 8 & 0xffffu, e2}; // refPic, refIdx, 0, 0 | mv
		if (both) rec[1] = (v2u){e[3], e[4]};
	}
	const gv2u *imot = (const gv2u *)(pkt + h->motion_off); // (section offsets and sizes are multiples of 8)
	for (uint32_t i = t; i < (mot >> 3); i += nt) ((gv2u *)omot)[i] = imot[i];
}

} // namespace
#endif
