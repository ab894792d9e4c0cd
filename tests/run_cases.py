"""Version-4 packets with RUNS in them: edge264_amd/synth.py draws every vector at random, so its pictures hold almost no two equal neighbours, which is
all the third level of the wire form (version 7, include/edge264_compact.h) is about.  plant() rewrites chosen macroblocks of a synthetic packet so that
they are equal to their left neighbour, or just not; CASES are the shapes tests/test_compact3.py (host) and tests/test_hip_wire3.py (MI355X) share, each
the smallest that reaches a distinct path of the fold and of the expansion."""
import numpy as np

from edge264_amd import backend, packet as P, synth

PLAIN = P.MBF_EDGE_LEFT | P.MBF_EDGE_TOP | P.MBF_DEBLOCK


def _uniform(mo, kind, donors):
    """one partition per list: every used list takes the reference and the vector of its first used quadrant, or a donor's; kind: None (the lists the
    macroblock has), "l0", "l1", "both" """
    mv = mo["mvs"].view("<i4")
    for l in range(2):
        used = [q for q in range(4) if mo["refPic"][l * 4 + q] >= 0]
        want = bool(used) if kind is None else kind in (("l0", "both"), ("l1", "both"))[l]
        if not want:
            mo["refPic"][l * 4:l * 4 + 4] = mo["refIdx"][l * 4:l * 4 + 4] = -1
            mv[l * 16:l * 16 + 16] = 0
            continue
        if used:
            rp, ri, v = mo["refPic"][l * 4 + used[0]], mo["refIdx"][l * 4 + used[0]], mv[l * 16 + used[0] * 4]
        else:
            assert donors[l] is not None, f"no macroblock of the picture predicts from list {l}"
            rp, ri, v = donors[l]
        mo["refPic"][l * 4:l * 4 + 4], mo["refIdx"][l * 4:l * 4 + 4] = rp, ri
        mv[l * 16:l * 16 + 16] = v


def plant(pkt: bytes, ops) -> bytes:
    """A version-4 packet with some inter macroblocks rewritten.  Every macroblock keeps its own motion record (the section is laid out again, in macroblock
    order), its own payload and, unless said otherwise, its own residual.  ops, applied in order:
      ("run", y, x0, x1[, kind])  macroblock x0 becomes a plain one (one partition per list -- kind None: the lists it has; "l0", "l1", "both" --, no residual,
                                  no flag but the edge ones); its flags, QPs, slice, dbk_slice and motion go over x0+1 .. x1, which lose their residual
      ("tail", y, x, xs)          x takes the head of xs (edge flags, QPs, slices, motion) and has the residual it had in `pkt`, which must be one
      ("full", y, x)              one vector of x moves by a sample: more than one partition, a full record at every level
      ("l0_of", y, x, xs)         x becomes xs without its list 1 (xs predicts from both)
      ("copy", y, x, ys, xs)      x becomes the plain macroblock (xs, ys) of another row
    The result passes e264hip_packet_check."""
    p = P.Packet(pkt)
    wm, n = p.width_mbs, len(p.mbs)
    mbs, mo = p.mbs.copy(), p.motion.copy()
    inter = mbs["kind"] == P.MB_INTER
    donors = []
    for l in range(2):
        a = np.nonzero(inter & (mo["refPic"][:, l * 4] >= 0))[0]
        donors.append(None if not len(a) else (mo["refPic"][a[0], l * 4], mo["refIdx"][a[0], l * 4], mo["mvs"][a[0]].view("<i4")[l * 16]))

    def head(dst, src):
        mbs["flags"][dst] = mbs["flags"][src] & PLAIN | mbs["flags"][dst] & (PLAIN ^ 0xff)
        for f in ("qp", "slice", "dbk_slice"):
            mbs[f][dst] = mbs[f][src]
        mo[dst] = mo[src]

    for op, y, x, *rest in ops:
        a = y * wm + x
        touched = [a]
        if op == "run":
            x1, kind = rest[0], rest[1] if len(rest) > 1 else None
            touched = list(range(a, y * wm + x1 + 1))
            assert x < x1 < wm
            _uniform(mo[a], kind, donors)
            for d in touched:
                mbs["flags"][d] &= PLAIN
                mbs["coded"][d] = mbs["nz_mask"][d] = 0
                if d != a:
                    head(d, a)
        elif op == "tail":
            assert p.mbs["coded"][a] != 0
            mbs["coded"][a], mbs["nz_mask"][a], mbs["flags"][a] = p.mbs["coded"][a], p.mbs["nz_mask"][a], p.mbs["flags"][a]  # (a run before may have taken them)
            head(a, y * wm + rest[0])
        elif op == "full":
            l = 0 if mo["refPic"][a, 0] >= 0 else 1
            assert mo["refPic"][a, l * 4] >= 0
            assert not mbs["flags"][a] & P.MBF_T8x8  # (no 8x8 transform over partitions below 8x8)
            mo["mvs"][a, l * 32] += 4
        elif op == "l0_of":
            head(a, y * wm + rest[0])
            mbs["flags"][a] &= PLAIN
            mbs["coded"][a] = mbs["nz_mask"][a] = 0
            assert mo["refPic"][a, 0] >= 0 and mo["refPic"][a, 4] >= 0
            _uniform(mo[a], "l0", donors)
        elif op == "copy":
            src = rest[0] * wm + rest[1]
            assert mbs["coded"][src] == 0 and not mbs["flags"][src] & (PLAIN ^ 0xff)
            head(a, src)
            mbs["flags"][a] &= PLAIN
            mbs["coded"][a] = mbs["nz_mask"][a] = 0
        else:
            raise ValueError(op)
        assert inter[touched].all(), (op, y, x)
    # the packet again: records, the motion section in macroblock order, the payload where it was from its start
    h = p.hdr.copy()
    mot = bytearray()
    refs = 0
    for a in np.nonzero(inter)[0]:
        rec, mh = P.motion_compact(mo[a])
        mbs["modes"][a] = np.frombuffer(np.array([len(mot), mh], "<u4").tobytes(), np.uint8)
        mot += rec
        for r in mo["refPic"][a]:
            if r >= 0:
                refs |= 1 << int(r)
    mbs_off = int(h["mbs_off"])
    motion_off = P.align16(mbs_off + 32 * n)
    payload_off = P.align16(motion_off + len(mot))
    pay = bytes(p.data[p.payload_off:p.payload_off + int(h["payload_bytes"])])
    h["motion_off"], h["payload_off"], h["total_bytes"], h["ref_slots"] = motion_off, payload_off, payload_off + len(pay), refs
    out = bytearray(payload_off + len(pay))
    out[:mbs_off] = p.data[:mbs_off]
    out[:P.FRAME_HDR.itemsize] = h.tobytes()
    out[mbs_off:mbs_off + 32 * n] = mbs.tobytes()
    out[motion_off:motion_off + len(mot)] = mot
    out[payload_off:] = pay
    out = bytes(out)
    assert backend.packet_check(out) == 0, backend.last_error()
    return out


def _residual_columns(pkt, y, lo, hi, both=None):
    """columns lo .. hi - 1 of row y whose macroblock is inter with residual (both: and predicts / does not predict from both lists)"""
    p = P.Packet(pkt)
    out = []
    for x in range(lo, hi):
        a = y * p.width_mbs + x
        if p.mbs["kind"][a] == P.MB_INTER and p.mbs["coded"][a] and (both is None or both == bool(p.motion["refPic"][a, 0] >= 0 and p.motion["refPic"][a, 4] >= 0)):
            out.append(x)
    return out


# name -> (width, height in macroblocks, synth seed and options, picture types, {picture index: ops})
# every macroblock of a P or B picture is inter (plant() rewrites inter macroblocks only); the I picture in front gives the references
_INTER = dict(place=lambda x, y, w, h: "inter")
CASES = {
    # no repeat possible
    "1x1": (1, 1, dict(seed=71, p_skip=1.0, **_INTER), "IPB", {}),
    # a run across the word boundary 31 -> 32 that also ends at the row's last macroblock; row 1 starts with what row 0 ends with (not a repeat); a run in word 0
    # (no deblocking: no edge flags, so that macroblocks of different rows can be equal at all)
    "33x3": (33, 3, dict(seed=72, p_skip=0.5, residual_prob=0.6, deblock=False, **_INTER), "IPB",
             {1: [("run", 0, 29, 32), ("copy", 1, 0, 0, 32), ("run", 1, 0, 3), ("run", 2, 5, 9)],
              2: [("run", 0, 30, 32, "both"), ("copy", 1, 0, 0, 32), ("run", 1, 0, 1), ("run", 2, 31, 32, "l1")]}),
    # 20 .. 64: word 1 is all repeats, the source two words back; 1 .. 64: the whole row but its first macroblock (0 .. 64 in the B picture)
    "65x2": (65, 2, dict(seed=73, p_skip=0.5, residual_prob=0.6, **_INTER), "IPB",
             {1: [("run", 0, 20, 64), ("run", 1, 1, 64)], 2: [("run", 0, 20, 64, "both"), ("run", 1, 0, 64, "l1")]}),
    # several slices; list-0, list-1 and two-list runs; runs cut by a full record and by a tail entry of the same head; a one-list entry in front of a
    # two-list entry with the same first 12 bytes (filled in by cases(): the columns with residual are looked up)
    "20x6": (20, 6, dict(seed=74, p_skip=0.3, residual_prob=0.9, slices_per_frame=3, num_refs=2, **_INTER), "IPBB", None),
}
_made = {}


def _ops_20x6(pkt, b_picture):
    if not b_picture:
        t = _residual_columns(pkt, 2, 4, 16)[0]
        return [("run", 0, 1, 6), ("run", 0, 7, 9), ("run", 1, 0, 19), ("run", 2, 1, 19), ("tail", 2, t, 1), ("run", 3, 2, 15), ("full", 3, 10),
                ("run", 5, 17, 19)]
    t = _residual_columns(pkt, 3, 4, 16, both=True)[0]
    return [("run", 0, 2, 8, "l0"), ("run", 1, 3, 12, "l1"), ("run", 2, 0, 19, "both"), ("run", 3, 1, 19, "both"), ("tail", 3, t, 1),
            ("run", 4, 6, 10, "both"), ("l0_of", 4, 5, 6), ("run", 5, 0, 7, "l1"), ("run", 5, 8, 15, "l0")]


def cases():
    """{name: [(picture type, version-4 packet, ops planted in it)]}, made once"""
    if not _made:
        for name, (w, h, kw, gop, ops) in CASES.items():
            g = synth.StreamSynth(w, h, **kw)
            out = []
            for i, ft in enumerate(gop):
                pkt = bytes(g.next_frame(ft))
                mine = [] if ft == "I" else ops[i] if ops is not None and i in ops else _ops_20x6(pkt, ft == "B") if ops is None else []
                out.append((ft, plant(pkt, mine) if mine else pkt, mine))
            _made[name] = out
    return _made


def streams(k=2):
    """the cases as packet lists for a device run: [name, [stream][picture]]; every stream of a case holds the same pictures"""
    return [(name, [[p for _, p, _ in pics] for _ in range(k)]) for name, pics in cases().items()]


def expected_repeats(ops, wm):
    """{(x, y)} the fold must make repeats, from the ops alone: x0+1 .. x1 of every run, less what a later op rewrote"""
    rep = set()
    for op, y, x, *rest in ops:
        if op == "run":
            rep |= {(c, y) for c in range(x + 1, rest[0] + 1)}
            rep.discard((x, y))  # (the start of a run planted over the end of an earlier one is not known to repeat)
        elif op in ("tail", "full"):
            rep.discard((x, y))
            rep.discard((x + 1, y))  # (its right neighbour no longer equals its left one)
        elif op in ("l0_of", "copy"):
            rep.discard((x, y))
            rep.discard((x + 1, y))
    return rep
