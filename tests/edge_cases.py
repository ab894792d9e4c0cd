"""Counts, from the packet alone (edge264_amd/packet.py), how often a picture reaches each range end the kernels carry special
arithmetic for.  The edge tests assert their packets contain the edge they are named after, so a later change to the generator cannot
drop one without a test noticing."""
from collections import Counter

import numpy as np

from edge264_amd import packet as P

# normAdjust8x8 (H.264 Table 8-13 / 8.5.13.1), by the position classes of oracle/e264_oracle.c norm_adjust8x8
_V8 = ((20, 18, 32, 19, 25, 24), (22, 19, 35, 21, 28, 26), (26, 23, 42, 24, 33, 31),
       (28, 25, 45, 26, 35, 33), (32, 28, 51, 30, 40, 38), (36, 32, 58, 34, 46, 43))


def _class8(pos):
    i, j = pos >> 3, pos & 7
    if i & 3 == 0 and j & 3 == 0:
        return 0
    if i & 1 and j & 1:
        return 1
    if i & 3 == 2 and j & 3 == 2:
        return 2
    if (i & 3 == 0 and j & 1) or (i & 1 and j & 3 == 0):
        return 3
    if (i & 3 == 0 and j & 3 == 2) or (i & 3 == 2 and j & 3 == 0):
        return 4
    return 5


NORM8 = np.array([[_V8[m][_class8(p)] for p in range(64)] for m in range(6)], np.int64)
INT16_ENDS = (32767, -32768, -32767)


def levels(pk, a):
    """(luma_dc, chroma_dc, {luma block: levels}, {chroma block: levels}, byte form) of macroblock a, read back from the payload in
    the order PacketBuilder.set_mb / the C emitters write it"""
    m = pk.mbs[a]
    coded, flags = int(m["coded"]), int(m["flags"])
    o = pk.payload_off + int(m["payload_off"])
    buf = pk.data
    if m["kind"] == P.MB_PCM:
        o += 384
    ldc = cdc = None
    if coded & P.CODED_LUMA_DC:
        ldc = np.frombuffer(buf, "<i2", 16, o)
        o += 32
    if coded & P.CODED_CHROMA_DC:
        cdc = np.frombuffer(buf, "<i2", 8, o)
        o += 16
    lev8 = bool(flags & P.MBF_LEV8)
    dt, sz = ("i1", 1) if lev8 else ("<i2", 2)
    n = 64 if flags & P.MBF_T8x8 and m["kind"] != P.MB_I16x16 else 16
    luma, chroma = {}, {}
    for k in range(16):
        if coded >> k & 1:
            luma[k] = np.frombuffer(buf, dt, n, o).astype(np.int32)
            o += n * sz
    for k in range(8):
        if coded >> (16 + k) & 1:
            chroma[k] = np.frombuffer(buf, dt, 16, o).astype(np.int32)
            o += 16 * sz
    return ldc, cdc, luma, chroma, lev8


def census(pkt) -> Counter:
    pk = P.Packet(bytes(pkt))
    c = Counter()
    mo = pk.motion
    for si, s in enumerate(pk.slices):
        if s["slice_type"] != 2 and s["weighted_bipred_idc"] == 1:
            c[f"luma_denom{int(s['luma_log2_weight_denom'])}"] += 1
            c[f"chroma_denom{int(s['chroma_log2_weight_denom'])}"] += 1
    for a, m in enumerate(pk.mbs):
        kind, flags = int(m["kind"]), int(m["flags"])
        if kind == P.MB_ABSENT:
            continue
        s = pk.slices[int(m["slice"])]
        if kind == P.MB_INTER:
            wd = (int(s["luma_log2_weight_denom"]), int(s["chroma_log2_weight_denom"]), int(s["chroma_log2_weight_denom"]))
            rp, ri = mo["refPic"][a], mo["refIdx"][a]
            mv = mo["mvs"][a].reshape(2, 16, 2)
            for q in range(4):
                used = [l for l in (0, 1) if rp[l * 4 + q] >= 0]
                for l in used:
                    if (np.abs(mv[l, q * 4:q * 4 + 4].astype(np.int32)) >= 30000).any():
                        c["mv_ends"] += 1
                if s["weighted_bipred_idc"] != 1:
                    continue
                ws = [[int(s["explicit_weights"][pl, l * 32 + ri[l * 4 + q]]) for pl in range(3)] for l in used]
                os_ = [[int(s["explicit_offsets"][pl, l * 32 + ri[l * 4 + q]]) for pl in range(3)] for l in used]
                if any(w[pl] == 128 and wd[pl] == 7 for w in ws for pl in range(3)):
                    c["denom7_default"] += 1
                if any(o in (-128, 127) for ol in os_ for o in ol):
                    c["offset_ends"] += 1
                if any(w in (-128, 127) for wl in ws for w in wl):
                    c["weight_ends"] += 1
                if len(used) == 2:
                    if any(ws[0][pl] & ws[1][pl] == 128 for pl in range(3)):
                        c["bipred_and128"] += 1
                    if any((ws[0][pl] == 128) != (ws[1][pl] == 128) and ws[0][pl] & ws[1][pl] != 128 for pl in range(3)):
                        c["default_beside_explicit"] += 1
        if kind != P.MB_PCM and int(m["coded"]):
            ldc, cdc, luma, chroma, lev8 = levels(pk, a)
            inter = int(kind == P.MB_INTER)
            qp = int(m["qp"][0])
            if flags & P.MBF_T8x8 and kind != P.MB_I16x16 and qp >= 36 and luma:
                LS = s["weightScale8x8"][inter].astype(np.int64) * NORM8[qp % 6]
                wraps = (LS << (qp // 6 - 6)) > 32767
                c["dequant8_wrap"] += int(sum(((blk != 0) & wraps).sum() for blk in luma.values()))
            ac = list(luma.values()) + list(chroma.values())
            if lev8:
                if any((b == -128).any() for b in ac):
                    c["lev8_m128"] += 1
                if any((b == 127).any() for b in ac):
                    c["lev8_127"] += 1
            elif any(np.isin(b, INT16_ENDS).any() for b in ac):
                c["int16_ac_ends"] += 1
            if ldc is not None and np.isin(ldc, INT16_ENDS).any():
                c["int16_luma_dc_ends"] += 1
            if cdc is not None and np.isin(cdc, INT16_ENDS).any():
                c["int16_chroma_dc_ends"] += 1
            if qp >= 48 and (s["weightScale4x4"] >= 200).any() and (luma or ldc is not None) and not flags & P.MBF_T8x8:
                c["dequant4_qp48_big_scale"] += 1
        if flags & P.MBF_DEBLOCK:
            offA, offB = int(s["FilterOffsetA"]), int(s["FilterOffsetB"])
            for pl in range(3):
                q = int(m["qp"][pl])
                qs = [q]
                if flags & P.MBF_EDGE_LEFT:
                    qs.append((q + int(pk.mbs[a - 1]["qp"][pl]) + 1) >> 1)
                if flags & P.MBF_EDGE_TOP:
                    qs.append((q + int(pk.mbs[a - pk.width_mbs]["qp"][pl]) + 1) >> 1)
                if any(not 0 <= x + offA <= 51 for x in qs):
                    c["indexA_clamp"] += 1
                if any(not 0 <= x + offB <= 51 for x in qs):
                    c["indexB_clamp"] += 1
                if pl and len(qs) > 1 and not 0 <= min(qs[1:]) + offA and (kind == P.MB_PCM or any(
                        pk.mbs[a - d]["kind"] == P.MB_PCM for d, f in ((1, P.MBF_EDGE_LEFT), (pk.width_mbs, P.MBF_EDGE_TOP)) if flags & f)):
                    c["pcm_chroma_edge_clamp"] += 1
    return c


def stream_census(pkts) -> Counter:
    total = Counter()
    for p in pkts:
        total.update(census(p))
    return total


ALL_I = (P.MB_I8x8, P.MB_I4x4, P.MB_I16x16)
FULL = dict(weight_range=(-128, 127), offset_range=(-128, 127))
# (name, picture types, generator options, census keys that must be counted)
CASES = [
    *[(f"denom{d}", "IPBBP", dict(weighted=1, slices_per_frame=2, weight_denoms=[(d, 7 - d), (d, d)], weight_pins=0.2, **FULL),
       [f"luma_denom{d}", f"chroma_denom{d}"]) for d in range(8)],
    ("denom7_and128", "IPBBPBB", dict(weighted=1, weight_denoms=[(7, 7)], weight_pins=0.5, t8x8=True),
     ["denom7_default", "bipred_and128", "default_beside_explicit", "offset_ends", "weight_ends"]),
    ("denom7_beside_others", "IPBBP", dict(weighted=1, slices_per_frame=3, weight_denoms=[(7, 0), (0, 7), (7, 2), (1, 7)], weight_pins=0.4, **FULL),
     ["denom7_default", "bipred_and128", "default_beside_explicit", "offset_ends", "weight_ends"]),
    ("weights_full_range", "IPBBP", dict(weighted=1, weight_denoms=[(d, 7 - d) for d in range(8)], weight_pins=0.3, t8x8=True, **FULL),
     ["offset_ends", "weight_ends"]),
    ("scaling8_qp48_intra", "II", dict(i_kinds=ALL_I, t8x8=True, scaling=True, scaling_range=(150, 256), qp_base=50, stress=True),
     ["dequant8_wrap"]),
    ("scaling8_qp48_inter", "IPBP", dict(t8x8=True, scaling=True, scaling_range=(150, 256), qp_base=50, stress=True, residual_prob=0.9),
     ["dequant8_wrap"]),
    ("scaling4_qp48", "IPB", dict(scaling=True, scaling_range=(1, 256), qp_base=50, stress=True, residual_prob=0.9),
     ["dequant4_qp48_big_scale"]),
    ("level_ends_intra", "II", dict(level_ends=True, i_kinds=ALL_I, t8x8=True),
     ["int16_ac_ends", "int16_luma_dc_ends", "int16_chroma_dc_ends", "lev8_m128", "lev8_127"]),
    ("level_ends_inter", "IPBP", dict(level_ends=True, t8x8=True, residual_prob=0.8, scaling=True, scaling_range=(150, 256), qp_base=50, stress=True),
     ["int16_ac_ends", "int16_chroma_dc_ends", "lev8_m128", "lev8_127", "dequant8_wrap"]),
    # int16 levels through the largest dequantisation factors: I16x16 / chroma DC and 4x4 blocks at QP 51 with entries >= 200, the 8x8 wrap
    ("level_ends_qp51_dc", "IIP", dict(level_ends=True, i_kinds=(P.MB_I16x16, P.MB_I4x4), scaling=True, scaling_range=(200, 256), qp_base=51,
                                       stress=True, intra_in_inter=0.3, residual_prob=0.9),
     ["int16_luma_dc_ends", "int16_chroma_dc_ends", "int16_ac_ends", "lev8_m128", "dequant4_qp48_big_scale"]),
    ("level_ends_qp51_t8", "IPB", dict(level_ends=True, i_kinds=ALL_I, t8x8=True, scaling=True, scaling_range=(200, 256), qp_base=51, stress=True,
                                       residual_prob=0.9),
     ["int16_ac_ends", "lev8_m128", "lev8_127", "dequant8_wrap"]),
    ("mv_ends", "IPBBP", dict(mv_ends=0.3, weighted=1, weight_denoms=[(7, 7)], weight_pins=0.3, t8x8=True),
     ["mv_ends", "denom7_default"]),
    ("filter_qp0", "IPB", dict(qp_base=0, stress=True, filter_offsets=(-12, -12), chroma_qp_offsets=(-12, -12), pcm_prob=0.3),
     ["indexA_clamp", "indexB_clamp", "pcm_chroma_edge_clamp"]),
    ("filter_qp51", "IPB", dict(qp_base=51, stress=True, filter_offsets=(12, 12), chroma_qp_offsets=(12, 12), pcm_prob=0.2),
     ["indexA_clamp", "indexB_clamp"]),
    ("filter_mixed", "IPB", dict(qp_base=0, stress=True, filter_offsets=(12, -12), chroma_qp_offsets=(12, -12), pcm_prob=0.3, slices_per_frame=2),
     ["indexB_clamp"]),
]
