"""Pictures for the prediction kernel's one-trip phases (e264_pred.h: pred_phase_setup / pred_phase_classify / pred_phase_residual): shared by
tests/test_pred_fetch_emu.py (the kernel's body on the host, and under the sanitizers in exact-size heap blocks) and tests/test_hip_pred_fetch.py (the device).

Every phase of the kernel requests all it may need before it looks at any of it, so what matters is (a) that every shape of motion record and every form
of residual payload is put together right from those requests and (b) that no request leaves what the macroblock owns: the motion section for the motion
(the pictures of tests/motion_fetch_cases.py), the macroblock's own payload for the residual -- most of all when the macroblock's payload is the packet's
last bytes, or its first.  The picture size is 17 x 5 macroblocks: two tiles wide, two tall, both partial -- the smallest picture with every tile boundary.

The payload pictures: an inter picture without residual (motion_fetch_cases.Directed) in which ONE macroblock gets the payload a case names and one other
macroblock an ordinary 4x4 luma block in two-byte form, so that the payload has a first and a last owner.  placement "last": the case's macroblock is the
picture's last, its payload the payload's last, and the packet is cut where that payload ends; "first": it is the picture's first, at payload offset 0."""
import functools

import numpy as np

from edge264_amd import packet as P
from tests import motion_fetch_cases as M

W, H = 17, 5
PLACEMENTS = ("last", "first")


def mb_payload_bytes(m) -> int:
    """bytes of payload a macroblock record owns (include/edge264_cmd.h e264_mb_payload_bytes)"""
    if int(m["kind"]) == P.MB_PCM:
        return 384
    coded, flags = int(m["coded"]), int(m["flags"])
    t8 = bool(flags & P.MBF_T8x8) and int(m["kind"]) != P.MB_I16x16
    ac = bin(coded >> 16 & 0xff).count("1") * 32 + (bin(coded & 0x1111).count("1") * 128 if t8 else bin(coded & 0xffff).count("1") * 32)
    return (32 if coded & P.CODED_LUMA_DC else 0) + (16 if coded & P.CODED_CHROMA_DC else 0) + (ac // 2 if flags & P.MBF_LEV8 else ac)


def _rebuild(raw: bytes, edit) -> bytes:
    """a version-4 packet put together again from its parsed parts after edit(builder)"""
    pk = P.Packet(raw)
    h = pk.hdr
    b = P.PacketBuilder(pk.width_mbs, pk.height_mbs, int(h["dst_slot"]), int(h["frame_id"]))
    b.slices = [s for s in np.array(pk.slices)]
    b.mbs = pk.mbs.copy()
    b.motion = pk.motion.copy()
    b.payload = bytearray()
    b.ref_slots = int(h["ref_slots"])
    edit(b)
    return b.finish()


def _trim(pkt: bytes) -> bytes:
    """the packet ends with the last byte a macroblock owns (the builder pads the payload to 16 bytes)"""
    buf = bytearray(pkt)
    hdr = np.frombuffer(buf, P.FRAME_HDR, 1)
    pk = P.Packet(pkt)
    end = max(int(m["payload_off"]) + mb_payload_bytes(m) for m in pk.mbs)
    hdr["payload_bytes"][0] = end
    hdr["total_bytes"][0] = int(hdr["payload_off"][0]) + end
    return bytes(buf[:int(hdr["total_bytes"][0])])


def _put(b, addr: int, data: bytes) -> None:
    while len(b.payload) % 8:
        b.payload.append(0)
    b.mbs[addr]["payload_off"] = len(b.payload)
    b.payload += data


def _ordinary(b, addr: int, rng) -> None:
    """one 4x4 luma block, two bytes per level"""
    m = b.mbs[addr]
    lev = rng.integers(-40, 41, 16).astype("<i2")
    lev[1] = 300  # (does not fit a byte)
    m["coded"], m["nz_mask"] = 1, 1
    m["flags"] &= ~(P.MBF_LEV8 | P.MBF_T8x8) & 255
    _put(b, addr, lev.tobytes())


def _chroma_dc_only(b, addr, rng):
    m = b.mbs[addr]
    dc = rng.integers(-30, 31, 8).astype("<i2")
    dc[0] |= 1
    m["coded"], m["nz_mask"] = P.CODED_CHROMA_DC, 0
    m["flags"] &= ~(P.MBF_LEV8 | P.MBF_T8x8) & 255
    _put(b, addr, dc.tobytes())


def _luma4x4_bytes(b, addr, rng):
    m = b.mbs[addr]
    k = 5
    lev = rng.integers(-128, 128, 16).astype("i1")
    lev[15] = -128
    m["coded"], m["nz_mask"] = 1 << k, 1 << k
    m["flags"] = (int(m["flags"]) & ~P.MBF_T8x8 & 255) | P.MBF_LEV8
    _put(b, addr, lev.tobytes())


def _luma8x8_bytes(b, addr, rng):
    m = b.mbs[addr]
    bq = 2
    lev = rng.integers(-128, 128, 64).astype("i1")
    lev[63] = 127
    m["coded"], m["nz_mask"] = 1 << (4 * bq), 0xf << (4 * bq)
    m["flags"] = int(m["flags"]) | P.MBF_LEV8 | P.MBF_T8x8
    _put(b, addr, lev.tobytes())


def _chroma_ac_no_dc(b, addr, rng):
    m = b.mbs[addr]
    blocks = b""
    for k in (2, 6):  # one block of Cb, one of Cr
        lev = rng.integers(-40, 41, 16).astype("<i2")
        lev[0], lev[15] = 0, 200
        blocks += lev.tobytes()
    m["coded"], m["nz_mask"] = 1 << (16 + 2) | 1 << (16 + 6), 0
    m["flags"] &= ~(P.MBF_LEV8 | P.MBF_T8x8) & 255
    _put(b, addr, blocks)


def _pcm(b, addr, rng):
    m = b.mbs[addr]
    m["kind"], m["coded"], m["nz_mask"], m["modes"] = P.MB_PCM, 0, 0xffff, 0
    m["qp"] = (0, int(m["qp"][1]), int(m["qp"][2]))
    m["flags"] &= ~(P.MBF_LEV8 | P.MBF_T8x8) & 255
    mo = b.motion[addr]
    mo["refPic"], mo["refIdx"], mo["mvs"] = -1, -1, 0
    _put(b, addr, rng.integers(0, 256, 384, dtype=np.uint8).tobytes())


PAYLOADS = {"chroma_dc_only": (_chroma_dc_only, 16), "luma4x4_bytes": (_luma4x4_bytes, 16), "luma8x8_bytes": (_luma8x8_bytes, 64),
            "chroma_ac_no_dc": (_chroma_ac_no_dc, 64), "pcm": (_pcm, 384)}  # (how it is made, the bytes it owns)


def special_addr(placement: str) -> int:
    return W * H - 1 if placement == "last" else 0


@functools.lru_cache(maxsize=None)
def payload_pictures():
    """[(name, frame type, packet)]: each payload case at each placement as an I, a P and a B picture (decode order)"""
    out = []
    for k, (name, (make, _)) in enumerate(PAYLOADS.items()):
        for j, placement in enumerate(PLACEMENTS):
            addr, other = special_addr(placement), special_addr(PLACEMENTS[1 - j])
            x, y = addr % W, addr // W
            g = M.Directed(W, H, (lambda mbx, mby, x=x, y=y: "uni" if (mbx, mby) == (x, y) else None), seed=4000 + 10 * k + j, decodable=True)
            rng = np.random.default_rng(900 + 10 * k + j)
            for ft in "IPB":
                pkt = g.next_frame(ft)
                if ft != "I":
                    def edit(b, make=make, addr=addr, other=other, placement=placement):
                        first, second = ((lambda: _ordinary(b, other, rng)), (lambda: make(b, addr, rng)))[::1 if placement == "last" else -1]
                        first()
                        second()
                    pkt = _trim(_rebuild(pkt, edit))
                out.append((f"{name}@{placement}", ft, pkt))
    return out


def motion_pictures(decodable=True):
    """the 17 x 5 pictures of tests/motion_fetch_cases.py; decodable=False: only the ones that differ, those with quadrants no list predicts"""
    pics = M.pictures(W, H, decodable=decodable)
    return pics if decodable else [(f"{n}_undecodable", ft, p) for n, ft, p in pics if n == "unused"]


def streams():
    """{case: its I, P, B packets}, every picture decodable"""
    out = {}
    for name, ft, pkt in list(motion_pictures()) + list(payload_pictures()):
        out.setdefault(name, []).append(pkt)
    return out
