"""Pictures for the parameter kernel's one-trip motion fetch (e264_dbkp.h: dbkp_fetch_list / dbkp_quad): shared by tests/test_motion_fetch_emu.py (the
kernel's body on the host, and under the sanitizers in exact-size heap blocks) and tests/test_hip_motion_fetch.py (the device).

The kernel requests everything a list's record MAY hold before it looks at any of it, so what matters is (a) that every shape of record is put together
right from those requests and (b) that no request leaves the packet's motion section, whatever shape the record has and wherever it lies -- most of all when
it is the section's LAST record and the section's end is the end of the packet.  A picture is drawn by synth.StreamSynth with the motion of chosen
macroblocks prescribed; relocate() then moves one macroblock's record to the end of the motion section (the directory in E264Mb.modes says where a record
lies: any order is a valid packet) and takes out the slack between the section and the payload."""
import functools

import numpy as np

from edge264_amd import packet as P, synth

SIZES = [(1, 1), (2, 1), (5, 3), (17, 5)]  # macroblocks; the last crosses a 64-macroblock workgroup and a 16 x 4 tile
DE_BRUIJN = [0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3]  # cyclic: every ordered pair of shapes follows one another once
LONGEST = [(True, 3, True, 3)] * 4  # both lists, four quadrants of four 4x4 vectors: 160 bytes
NMV = (1, 2, 2, 4)


def record_bytes(h: int) -> int:
    return sum(8 if h >> (8 + l) & 1 else sum(4 + 4 * NMV[h >> (10 + 2 * (l * 4 + q)) & 3] for q in range(4) if h >> (l * 4 + q) & 1) for l in range(2))


class Directed(synth.StreamSynth):
    """plan(mbx, mby) of every macroblock of a P or B picture: None (drawn as usual), "intra", "uni" (one partition, list 0: an 8-byte record) or four
    (used in list 0, its sub-partition shape, used in list 1, its shape), one per quadrant (list 1 only in B pictures)."""

    def __init__(self, w, h, plan, seed, decodable=False, **kw):
        self.plan, self.spec, self.decodable = plan, None, decodable  # decodable: a quadrant the plan leaves without a list is predicted from list 0
        super().__init__(w, h, seed=seed, place=self._place, residual_prob=0.0, intra_in_inter=0.0, mv_range=6, **kw)

    def _place(self, mbx, mby, W, H):
        self.spec = self.plan(mbx, mby)
        return "intra" if self.spec == "intra" else "inter"

    def _motion(self, ftype, l0, l1, t8):
        if self.spec is None:
            return super()._motion(ftype, l0, l1, t8)
        rng = self.rng
        refPic, refIdx, mvs = np.full(8, -1, np.int8), np.full(8, -1, np.int8), np.zeros((2, 16, 2), np.int16)

        def vec(*others):  # around the bS threshold of four quarter samples, different from `others`
            while True:
                v = tuple(int(x) for x in rng.integers(-6, 7, 2))
                if v not in others:
                    return v
        if self.spec == "uni":
            i = int(rng.integers(0, len(l0)))
            refIdx[:4], refPic[:4], mvs[0, :, :] = i, l0[i], vec()
            return dict(refPic=refPic, refIdx=refIdx, mvs=mvs)
        for lx, lst in ((0, l0), (1, l1)):
            for q in range(4):
                used, sub = self.spec[q][2 * lx], self.spec[q][2 * lx + 1]
                if self.decodable and lx == 0 and not (self.spec[q][2] and l1):
                    used = True
                if not lst or not used:
                    continue
                i = int(rng.integers(0, len(lst)))
                refIdx[lx * 4 + q], refPic[lx * 4 + q] = i, lst[i]
                a = vec()
                b = vec(a)
                c = vec(a, b)
                d = vec(a, b, c)
                mvs[lx, q * 4:q * 4 + 4] = [(a, a, a, a), (a, a, b, b), (a, b, a, b), (a, b, c, d)][sub]
        return dict(refPic=refPic, refIdx=refIdx, mvs=mvs)


def relocate(pkt: bytes, last_addr: int, align: int = 8) -> bytes:
    """The same picture with the record of macroblock last_addr as the LAST of the motion section and the section ending where that record ends (what slack
    `align` of the payload asks for lies in front of it).  Without payload the record's last byte is the packet's last."""
    buf = bytearray(pkt)
    hdr = np.frombuffer(buf, P.FRAME_HDR, 1)
    mo, po, total = int(hdr["motion_off"][0]), int(hdr["payload_off"][0]), int(hdr["total_bytes"][0])
    if not mo:
        return pkt
    n = int(hdr["width_mbs"][0]) * int(hdr["height_mbs"][0])
    mbs = np.frombuffer(buf, P.MB, n, int(hdr["mbs_off"][0]))
    recs = []
    for a in np.nonzero(mbs["kind"] == P.MB_INTER)[0]:
        off, h = (int(x) for x in np.frombuffer(mbs["modes"][a].tobytes(), "<u4"))
        recs.append((int(a), h, bytes(buf[mo + off:mo + off + record_bytes(h)])))
    assert any(a == last_addr for a, _, _ in recs), "the macroblock to end the section with is not inter"
    recs.sort(key=lambda r: r[0] == last_addr)  # (stable: the others keep their order)
    sec = bytearray()
    slack = -sum(len(r) for _, _, r in recs) % align
    for a, h, r in recs:
        if a == last_addr:
            sec += bytes([0xEE]) * slack
        mbs["modes"][a] = np.frombuffer(np.array([len(sec), h], "<u4").tobytes(), np.uint8)
        sec += r
    payload = bytes(buf[po:total])
    hdr["payload_off"][0] = mo + len(sec)
    hdr["total_bytes"][0] = mo + len(sec) + len(payload)
    out = bytes(buf[:mo]) + bytes(sec) + payload
    assert (mo + len(sec)) % 8 == 0 and len(out) == int(hdr["total_bytes"][0])
    return out


def shapes_plan(mbx, mby):
    """every sub-partition shape in every quadrant, beside and below every other one (a row of 17 holds all sixteen ordered pairs, and so do two rows)"""
    s = DE_BRUIJN[(mbx + mby) % 16]
    return [(True, (s + q) % 4, True, (s + q + 1 + mbx) % 4) for q in range(4)]


def unused_plan(mbx, mby):
    """quadrants that list 0, list 1, both or neither predict; macroblock (0, 0) is inter without anything"""
    use = [((mbx + 3 * mby + q) % 4 if (mbx, mby) != (0, 0) else 3) for q in range(4)]
    return [(u in (0, 2), (mbx + q) % 4, u in (1, 2), (mby + q) % 4) for u, q in zip(use, range(4))]


def placements(w, h):
    """where an end-of-section record is put: the picture's last macroblock, its first, and the records on both sides of a workgroup boundary (64 macroblocks)"""
    n = w * h
    out = {"last": n - 1}
    if n > 1:
        out["first"] = 0
    if n > 64:
        out["wg_end"], out["wg_start"] = 63, 64
    return out


def end_cases(w, h):
    """(name, plan, macroblock whose record ends the section)"""
    for where, addr in placements(w, h).items():
        x, y = addr % w, addr // w
        # the longest record there is (in a P picture: its list-0 half), every other macroblock inter without residual: the section's end is the packet's end
        yield f"longest@{where}", (lambda mbx, mby, x=x, y=y: LONGEST if (mbx, mby) == (x, y) else None), addr
        # the only inter macroblock of the picture, one partition: a motion section of 8 bytes
        yield f"only_inter@{where}", (lambda mbx, mby, x=x, y=y: "uni" if (mbx, mby) == (x, y) else "intra"), addr
        # a one-partition record last, behind records of every kind
        yield f"one_partition@{where}", (lambda mbx, mby, x=x, y=y: "uni" if (mbx, mby) == (x, y) else None), addr


@functools.lru_cache(maxsize=None)
def pictures(w, h, align=8, decodable=False):
    """[(name, frame type, packet)]: each case as an I, a P and a B picture (decode order), the P and B ones relocated.  decodable: for whole-picture decoding --
    no quadrant without any list (the parameter kernel has an answer for one, reference 0xff and vector 0 on both lists, but nobody defines its samples)"""
    out = []
    cases = [("shapes", shapes_plan, w * h - 1), ("unused", unused_plan, w * h - 1), *end_cases(w, h)]
    for k, (name, plan, addr) in enumerate(cases):
        g = Directed(w, h, plan, seed=1000 + 17 * k + w, decodable=decodable)
        for ft in "IPB":
            pkt = g.next_frame(ft)
            if ft != "I":
                pkt = relocate(pkt, addr, align)
            out.append((name, ft, pkt))
    return out
