"""The second level of the WIRE form (version 6, include/edge264_compact.h): the inter macroblock of one partition per list WITH residual as a 24- or 32-byte
entry -- E264MbCompact [+ E264MbCompactL1] + {coded, payload_off, nz_mask} -- found with a third bitmap and a third popcount.  tests/test_compact.py at
level 2, host side, no GPU: fold, unfold and refold byte for byte; every kind of entry occurs; the oracle and the kernels' own source (tests/emu) read the
expansion; damaged packets are refused or sound; the front end's own level-2 output; the sizes on the 1080p fixtures.  Version 5 is not touched: its tests
stay in tests/test_compact.py.  The -m gpu part is tests/test_hip_wire2.py."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, front, packet as P, synth
from oracle.pyoracle import Oracle, _dpb_array

HERE = os.path.dirname(os.path.abspath(__file__))
STREAMS = os.path.join(HERE, "golden", "streams")
SMALL = sorted(p for p in glob.glob(os.path.join(STREAMS, "*.264")) if os.path.getsize(p) < 60_000)
FIXTURES_1080 = ("nat1080_ipp30.264", "cabac_nat1080_ibbp30.264", "hd1080_ipp30.264", "cabac_hd1080_ibbp30.264")

MBF_T8x8, MBF_DONE, MBF_LEV8, MBCF_LIST1 = 0x01, 0x10, 0x20, 0x80


def _have_front():
    try:
        front.load()
        return True
    except front.FrontError:
        return False


needs_front = pytest.mark.skipif(not _have_front(), reason="front-end library not built (needs the reference tree)")


@pytest.fixture(scope="module")
def emu():
    d = os.path.join(HERE, "emu")
    subprocess.run(["make", "-C", d], check=True, stdout=subprocess.DEVNULL)
    pe = C.CDLL(os.path.join(d, "libe264_pred_emu.so"))
    ie = C.CDLL(os.path.join(d, "libe264_intra_emu.so"))
    pe.e264emu_expand.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
    pe.e264emu_set_expand.argtypes = [C.c_void_p]
    ie.e264emu_set_expand.argtypes = [C.c_void_p]
    pe.e264emu_pred_frame2.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    pe.e264emu_dbkparam_frame2.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    ie.e264emu_intra_frame2.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
    yield pe, ie
    pe.e264emu_set_expand(None)
    ie.e264emu_set_expand(None)


# the synthetic pictures (shared with tests/test_hip_wire2.py): two and three bitmap words per row, several slices, one macroblock, 8x8 transform and both level forms
SYNTH_CASES = ((31, 37, 5, "IPBB", dict(p_skip=0.6, residual_prob=0.9, num_refs=2)), (32, 65, 2, "IPB", dict(p_skip=0.7, residual_prob=0.8)),
               (33, 33, 3, "IPB", dict(slices_per_frame=3)), (34, 1, 1, "IPB", dict(p_skip=1.0, residual_prob=1.0)),
               (35, 37, 5, "IPBB", dict(t8x8=True, level_ends=True)))
_synth = None


def synth_packets():
    """[(name, version-4 packet)], made once"""
    global _synth
    if _synth is None:
        _synth = []
        for seed, w, h, gop, kw in SYNTH_CASES:
            g = synth.StreamSynth(w, h, seed=seed, **kw)
            _synth += [(f"synth{seed}", bytes(g.next_frame(ft))) for ft in gop]
    return _synth


def wire_cases():
    out = [(n, backend.packet_compact(p, level=2)) for n, p in synth_packets()]
    return [(n, w) for n, w in out if w[4] == 6]


def entries(wire: bytes):
    """The entries of a version-6 packet as the header comment of edge264_compact.h lays them out, read here without the C code:
    [(x, y, kind, flags, coded, nz_mask)], kind one of "full", "l0", "l1", "both", each with "+r" when the tail follows"""
    h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
    assert int(h["version"]) == 6
    wm, hm, base = int(h["width_mbs"]), int(h["height_mbs"]), int(h["mbs_off"])
    nc, nb, eb, wpr, nr, zero = (int(v) for v in np.frombuffer(wire, "<u4", 6, base))
    assert wpr == (wm + 31) // 32 and zero == 0
    tab = np.frombuffer(wire, "<u4", 3 * hm + 3 * hm * wpr, base + 24)
    row_off, bits = tab[:hm], tab[3 * hm:].reshape(3, hm, wpr)
    ent = base + ((24 + 12 * hm + 12 * hm * wpr + 7) & ~7)
    out = []
    for y in range(hm):
        pos = ent + int(row_off[y])
        for x in range(wm):
            c, b, r = (int(bits[k, y, x >> 5]) >> (x & 31) & 1 for k in range(3))
            assert c or not (b or r)
            if not c:
                m = np.frombuffer(wire, P.MB, 1, pos)[0]
                out.append((x, y, "full", int(m["flags"]), int(m["coded"]), int(m["nz_mask"]), int(m["kind"])))
                pos += 32
                continue
            flags = wire[pos]
            size = 12 + 8 * b + 12 * r
            coded = nz = 0
            if r:
                coded, _, nz, z = np.frombuffer(wire, np.dtype([("c", "<u4"), ("p", "<u4"), ("n", "<u2"), ("z", "<u2")]), 1, pos + size - 12)[0]
                assert z == 0
            out.append((x, y, ("both" if b else "l1" if flags & MBCF_LIST1 else "l0") + ("+r" if r else ""), flags & 0x7f, int(coded), int(nz), P.MB_INTER))
            pos += size
    assert pos - ent == eb == 32 * wm * hm - 20 * nc + 8 * nb + 12 * nr
    return out


def check_round_trip(name, pkt):
    """fold at level 2, unfold, refold: the packet's information and the wire bytes come back"""
    wire = backend.packet_compact(pkt, level=2)
    assert backend.packet_check(wire) == 0, (name, backend.last_error())
    back = backend.packet_expand(wire)
    assert backend.packet_check(back) == 0, (name, backend.last_error())
    assert backend.packet_compact(back, level=2) == wire, name  # the expansion is canonical
    a, b = P.Packet(pkt), P.Packet(back)
    for f in ("kind", "flags", "qp", "nz_mask", "slice", "coded", "dbk_slice"):
        assert np.array_equal(a.mbs[f], b.mbs[f]), (name, f)
    res = (a.mbs["coded"] != 0)
    assert np.array_equal(a.mbs["payload_off"][res], b.mbs["payload_off"][res]), name  # payload_off travels as it is
    ma, mb = a.motion, b.motion
    assert (ma is None) == (mb is None)
    if ma is not None:
        assert ma.tobytes() == mb.tobytes(), name
    assert bytes(a.data[a.payload_off:a.payload_off + int(a.hdr["payload_bytes"])]) == bytes(b.data[b.payload_off:b.payload_off + int(b.hdr["payload_bytes"])])
    assert P.Packet(wire).mbs.tobytes() == b.mbs.tobytes()  # P.Packet reads a version-6 packet through its expansion
    return wire


def test_fold_unfold_refold_synthetic():
    n6 = 0
    for name, pkt in synth_packets():
        assert backend.packet_check(pkt) == 0
        wire = check_round_trip(name, pkt)
        w1 = backend.packet_compact(pkt)  # level 1 still gives version 5 ...
        assert w1[4] == 5 and w1 == backend.packet_compact(pkt, level=1)
        assert wire[4] == 6  # ... and level 2 version 6, whatever the picture holds
        n6 += 1
    assert n6 == sum(len(c[3]) for c in SYNTH_CASES)


def test_every_kind_of_entry_occurs():
    seen = {}
    for name, wire in wire_cases():
        for x, y, kind, flags, coded, nz, mbk in entries(wire):
            if mbk != P.MB_INTER:
                continue
            seen[kind] = seen.get(kind, 0) + 1
            if kind.endswith("+r"):
                for tag, on in (("t8x8", flags & MBF_T8x8), ("no_t8x8", not flags & MBF_T8x8), ("lev8", flags & MBF_LEV8), ("no_lev8", not flags & MBF_LEV8)):
                    seen[tag] = seen.get(tag, 0) + bool(on)
                assert coded or nz or flags & (MBF_T8x8 | MBF_LEV8), name  # a tail only where it says something
            elif kind != "full":
                assert not coded and not nz and not flags & (MBF_T8x8 | MBF_LEV8), name
            assert kind == "full" or not flags & (MBF_DONE | 0x40)
    for k in ("l0+r", "l1+r", "both+r", "l0", "both", "full", "t8x8", "no_t8x8", "lev8", "no_lev8"):
        assert seen.get(k, 0) > 0, (k, seen)
    assert seen["l0+r"] + seen["l1+r"] > 200 and seen["both+r"] > 20, seen


def test_the_expansion_decodes_to_the_same_pictures():
    """the oracle (a version-4 reader) on the original packet and on level-2 fold + unfold: same pictures"""
    for seed, kw in ((41, dict(p_skip=0.5, residual_prob=0.9, num_refs=2)), (42, dict(p_skip=0.4, residual_prob=0.8, t8x8=True, level_ends=True))):
        g = synth.StreamSynth(9, 5, seed=seed, **kw)
        nb = P.frame_bytes(9, 5)
        rng = np.random.default_rng(1)
        dpb = [rng.integers(0, 256, nb + 16, dtype=np.uint8) for _ in range(6)] + [None] * 26
        dpb6 = [None if b is None else b.copy() for b in dpb]
        o4, o6 = Oracle(), Oracle()
        for ft in "IPPBP":
            pkt = bytes(g.next_frame(ft))
            o4.decode_frame(pkt, dpb, 3)
            wire = backend.packet_compact(pkt, level=2)
            assert wire[4] == 6
            o6.decode_frame(backend.packet_expand(wire), dpb6, 3)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            assert np.array_equal(dpb[d][:nb], dpb6[d][:nb])


@needs_front
def test_every_committed_stream_folds_and_unfolds():
    saved = 0
    for f in sorted(glob.glob(os.path.join(STREAMS, "*.264"))):
        if os.path.getsize(f) > 400_000:
            continue
        for pkt in front.capture_packets(open(f, "rb").read())[0]:
            pkt = bytes(pkt)
            wire = check_round_trip(f, pkt)
            saved += len(pkt) - len(wire)
    assert saved > 0


def _held_against_host_expansion(pe, name, wire, grids):
    back = backend.packet_expand(wire)
    h = np.frombuffer(back, P.FRAME_HDR, 1)[0]
    want = back[int(h["mbs_off"]):int(h["payload_off"])]
    for nt in grids:
        area = (C.c_uint8 * (len(want) + 64))()
        C.memset(area, 0xA5, len(want) + 64)
        pe.e264emu_expand(wire, area, nt)
        assert bytes(area[:len(want)]) == want, (name, nt)
        assert bytes(area[len(want):]) == b"\xa5" * 64, (name, nt)  # nothing behind e264_expand_area_bytes


def test_expand_kernel_source_equals_the_host_expansion(emu):
    """e264_expand.h run thread by thread on the host: the record array and the motion section it writes are the bytes of e264_expand_packet"""
    pe, _ = emu
    cases = wire_cases()
    assert len(cases) >= 16
    for name, wire in cases:
        _held_against_host_expansion(pe, name, wire, (256, 64 * 7, 1))


@needs_front
def test_expand_kernel_source_on_large_pictures(emu):
    """1080p packets of the encoder-shaped streams (120 x 68 macroblocks: four bitmap words per row), P and B pictures"""
    pe, _ = emu
    n = 0
    for name in ("nat1080_ipp30.264", "cabac_nat1080_ibbp30.264"):
        pk = front.capture_packets(open(os.path.join(STREAMS, name), "rb").read())[0]
        for p in pk[1:8:3]:
            wire = check_round_trip(name, bytes(p))
            assert wire[4] == 6
            _held_against_host_expansion(pe, name, wire, (256, 64 * 7, 1))
            n += 1
    assert n == 6


def test_kernels_read_a_version6_packet_through_its_expansion(emu):
    """the four kernels' source on (version-6 packet + expansion buffer) against the same source on the version-4 packet: identical pictures and parameters"""
    pe, ie = emu
    n = 0
    for seed, w, h, kw in ((51, 20, 6, dict(p_skip=0.6, num_refs=2, residual_prob=0.9)), (52, 7, 5, dict(p_skip=0.5, intra_in_inter=0.2, t8x8=True, level_ends=True))):
        g = synth.StreamSynth(w, h, seed=seed, **kw)
        nb = P.frame_bytes(w, h)
        rng = np.random.default_rng(seed)
        dpb = [rng.integers(0, 256, nb + 64, dtype=np.uint8) for _ in range(6)] + [None] * 26
        for ft in "IPPB":
            pkt = bytes(g.next_frame(ft))
            wire = backend.packet_compact(pkt, level=2)
            assert wire[4] == 6
            n += sum(1 for e in entries(wire) if e[2].endswith("+r"))
            res = []
            for form in (pkt, wire):
                mine = [None if b is None else b.copy() for b in dpb]
                scratch = np.full(146 * w * h + 64, 0x5A, np.uint8)
                prm = np.zeros(144 * w * h + 64, np.uint8)
                area = None
                if form is wire:
                    back = backend.packet_expand(wire)
                    hb = np.frombuffer(back, P.FRAME_HDR, 1)[0]
                    area = (C.c_uint8 * (int(hb["payload_off"]) - int(hb["mbs_off"])))()
                    pe.e264emu_expand(wire, area, 256)
                pe.e264emu_set_expand(area)
                ie.e264emu_set_expand(area)
                arr = _dpb_array(mine)
                assert pe.e264emu_pred_frame2(form, arr, scratch.ctypes.data) == 0
                assert ie.e264emu_intra_frame2(form, arr, scratch.ctypes.data, 1) == 0
                assert pe.e264emu_dbkparam_frame2(form, prm.ctypes.data, None) == 0
                d = int(P.Packet(pkt).hdr["dst_slot"])
                res.append((mine[d][:nb].copy(), prm[:144 * w * h].copy()))
            pe.e264emu_set_expand(None)
            ie.e264emu_set_expand(None)
            assert np.array_equal(res[0][0], res[1][0])
            assert np.array_equal(res[0][1], res[1][1])
            Oracle().decode_frame(pkt, dpb, 3)  # the next picture's references
    assert n > 100  # (residual entries went through the kernels)


def test_damaged_version6_packets_are_refused_or_sound():
    """bytes of the table, the entries and the header damaged at random: e264hip_packet_check either refuses the packet or its expansion is a sound
    version-4 packet (what the device unfolds is what was vetted)"""
    rng = np.random.default_rng(6)
    refused = accepted = 0
    for name, wire in wire_cases():
        h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
        lo, hi = 0, int(h["payload_off"])
        for _ in range(150):
            buf = bytearray(wire)
            for _ in range(int(rng.integers(1, 4))):
                i = int(rng.integers(lo, hi))
                buf[i] = int(rng.integers(0, 256)) if rng.random() < 0.6 else buf[i] ^ (1 << int(rng.integers(0, 8)))
            buf = bytes(buf)
            if backend.packet_check(buf) != 0:
                refused += 1
                continue
            accepted += 1
            assert backend.packet_check(backend.packet_expand(buf)) == 0
    assert refused > 100 and accepted > 100


def test_wrong_form_inputs_are_refused():
    name, wire = wire_cases()[1]  # (a P picture)
    assert backend.packet_check(wire[:-8]) != 0
    assert backend.packet_check(wire[:100]) != 0
    for v in (5, 4):  # a version-6 packet relabelled
        other = bytearray(wire)
        other[4] = v
        assert backend.packet_check(bytes(other)) != 0, v
    for level in (1, 2):
        with pytest.raises(backend.BackendError):
            backend.packet_compact(wire, level=level)  # already folded
        with pytest.raises(backend.BackendError):
            backend.packet_compact(backend.packet_compact(synth_packets()[1][1]), level=level)  # ... at level 1
    for level in (3, 0, -1):
        with pytest.raises(backend.BackendError, match="level"):
            backend.packet_compact(synth_packets()[1][1], level=level)
    # spare bits of an entry: the tail's `zero`, and a flag an entry may not carry
    ent = [e for e in entries(wire)]
    h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
    hm, wpr = int(h["height_mbs"]), (int(h["width_mbs"]) + 31) // 32
    pos = int(h["mbs_off"]) + ((24 + 12 * hm + 12 * hm * wpr + 7) & ~7)
    for x, y, kind, *_ in ent:
        size = 32 if kind == "full" else 12 + (8 if kind.startswith("both") else 0) + (12 if kind.endswith("+r") else 0)
        if kind.endswith("+r"):
            for at, bit in ((pos + size - 2, 1), (pos + size - 1, 0x80), (pos, 0x40), (pos, MBF_DONE)):
                bad = bytearray(wire)
                bad[at] |= bit
                assert backend.packet_check(bytes(bad)) != 0, (kind, at - pos, bit)
            break
        pos += size
    else:
        raise AssertionError("no residual entry")


@needs_front
def test_front_end_emits_the_same_version6_packets():
    """e264front_set_compact(2): what leaves the front end is the level-2 fold of what it would have sent (pictures without inter macroblocks leave as version 4)"""
    n6 = n4 = 0
    for f in SMALL:
        data = open(f, "rb").read()
        plain = [bytes(p) for p in front.capture_packets(data)[0]]
        wire = [bytes(p) for p in front.capture_packets(data, compact=2)[0]]
        assert len(plain) == len(wire), f
        for a, b in zip(plain, wire):
            assert backend.packet_check(b) == 0
            if b[4] == 6:
                assert b == backend.packet_compact(a, level=2), f
                n6 += 1
            else:
                assert a == b and int(P.Packet(a).hdr["n_inter_mbs"]) == 0, f
                n4 += 1
    front.capture_packets(b"", compact=False)  # (the switch is global to the library: leave it off)
    assert n6 > 50 and n4 > 0


@needs_front
def test_front_end_folds_pictures_that_leave_in_several_packets():
    """damaged streams (a slice cut short and sent again: the picture goes out in several packets whose records are edited in the packet before they are
    folded): packet by packet the level-2 fold of what the front end sends with the option off"""
    from tests import damage
    n6 = multi = 0
    for c in damage.RESENT[:10]:
        data = damage.truncated_then_resent(*c)
        plain = [bytes(p) for p in front.capture_packets(data)[0]]
        wire = [bytes(p) for p in front.capture_packets(data, compact=2)[0]]
        assert len(plain) == len(wire)
        seen = {}
        for a, b in zip(plain, wire):
            assert backend.packet_check(b) == 0
            fid = int(P.Packet(a).hdr["frame_id"])
            seen[fid] = seen.get(fid, 0) + 1
            if b[4] == 6:
                assert b == backend.packet_compact(a, level=2)
                n6 += 1
            else:
                assert a == b
        multi += sum(1 for v in seen.values() if v > 1)
    front.capture_packets(b"", compact=False)
    assert n6 > 20 and multi > 5


@needs_front
@pytest.mark.parametrize("name", FIXTURES_1080)
def test_sizes_on_the_1080p_fixtures(name):
    """level 2 is never larger than level 1; on the encoder-shaped streams it is below 0.65 of version 4 (counted on the fixtures: 0.618 and 0.641 less one
    bitmap of a few hundred bytes per picture)"""
    pk = [bytes(p) for p in front.capture_packets(open(os.path.join(STREAMS, name), "rb").read())[0]]
    b4 = b5 = b6 = 0
    for p in pk:
        w5, w6 = backend.packet_compact(p), backend.packet_compact(p, level=2)
        b4, b5, b6 = b4 + len(p), b5 + len(w5), b6 + len(w6)
    print(f"{name}: v5/v4 {b5 / b4:.4f}  v6/v4 {b6 / b4:.4f}  ({b4} {b5} {b6} bytes, {len(pk)} packets)")
    assert b6 <= b5
    if name in ("nat1080_ipp30.264", "cabac_nat1080_ibbp30.264"):
        assert b6 < 0.65 * b4
