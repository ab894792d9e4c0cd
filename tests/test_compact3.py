"""The third level of the WIRE form (version 7, include/edge264_compact.h): a run of equal plain entries in a row travels as ONE entry and a bit per further
macroblock (a fourth bitmap, pbits; five popcounts find an entry; a repeat reads the entry of its source).  tests/test_compact2.py at level 3, host side,
no GPU: fold, unfold and refold byte for byte; the expansion is the level-2 expansion; the runs planted by tests/run_cases.py are where the fold must find
them; the kernels' own source (tests/emu) reads the expansion; damaged packets are refused or sound; every structure rule and the canonical rule broken by
hand; the front end's own level-3 output; the sizes on the 1080p fixtures.  Versions 5 and 6 are not touched: their tests stay where they are.  The -m gpu
part is tests/test_hip_wire3.py."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, front, packet as P
from oracle.pyoracle import Oracle, _dpb_array
from tests import run_cases
from tests.test_compact2 import synth_packets

HERE = os.path.dirname(os.path.abspath(__file__))
STREAMS = os.path.join(HERE, "golden", "streams")
SMALL = sorted(p for p in glob.glob(os.path.join(STREAMS, "*.264")) if os.path.getsize(p) < 60_000)
FIXTURES_1080 = ("nat1080_ipp30.264", "cabac_nat1080_ibbp30.264", "hd1080_ipp30.264", "cabac_hd1080_ibbp30.264")
MBCF_LIST1 = 0x80


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


def planted():
    """[(name, picture type, version-4 packet, ops)] of tests/run_cases.py"""
    return [(f"{name}/{i}{ft}", ft, pkt, ops) for name, pics in run_cases.cases().items() for i, (ft, pkt, ops) in enumerate(pics)]


def all_packets():
    """[(name, version-4 packet)]: the planted pictures and the random ones of tests/test_compact2.py (hardly a run in them)"""
    return [(n, p) for n, _, p, _ in planted()] + synth_packets()


def wire_cases():
    return [(n, backend.packet_fold(p, 3)) for n, p in all_packets()]


def layout(wire: bytes):
    """where the parts of a version-7 packet lie, from the header comment of edge264_compact.h: (wm, hm, wpr, offset of the table header, of row_off, of the
    four bitmaps [cbits, bbits, rbits, pbits], of the entry area)"""
    h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
    assert int(h["version"]) == 7
    wm, hm, base = int(h["width_mbs"]), int(h["height_mbs"]), int(h["mbs_off"])
    wpr = (wm + 31) // 32
    bits = base + 32 + 12 * hm
    return wm, hm, wpr, base, base + 32, [bits + 4 * k * hm * wpr for k in range(4)], base + ((32 + 12 * hm + 16 * hm * wpr + 7) & ~7)


def entries(wire: bytes):
    """The macroblocks of a version-7 packet as the header comment of edge264_compact.h lays them out, read here without the C code: a list in raster order
    of dicts x, y, kind ("full", "l0", "l1", "both", each with "+r" when the tail follows), repeat, pos (offset of the entry it reads: its own, or its
    source's), head (the 12 or 20 bytes of a compact entry), slice"""
    wm, hm, wpr, base, _, _, ent = layout(wire)
    nc, nb, eb, w_, nr, np_, nq, zero = (int(v) for v in np.frombuffer(wire, "<u4", 8, base))
    assert w_ == wpr and zero == 0
    tab = np.frombuffer(wire, "<u4", 3 * hm + 4 * hm * wpr, base + 32)
    row_off, row_cbase, row_bbase, bits = tab[:hm], tab[hm:2 * hm], tab[2 * hm:3 * hm], tab[3 * hm:].reshape(4, hm, wpr)
    out = []
    seen = dict(c=0, b=0, r=0, p=0, q=0)
    for y in range(hm):
        pos = ent + int(row_off[y])
        assert (int(row_cbase[y]), int(row_bbase[y])) == (seen["c"], seen["b"])
        src = None
        for x in range(wm):
            c, b, r, p = (int(bits[k, y, x >> 5]) >> (x & 31) & 1 for k in range(4))
            assert c or not (b or r or p)
            assert not (p and r)
            if not c:
                m = np.frombuffer(wire, P.MB, 1, pos)[0]
                out.append(dict(x=x, y=y, kind="full", repeat=False, pos=pos, head=None, slice=int(m["slice"]), mbkind=int(m["kind"])))
                pos += 32
                src = None
                continue
            seen["c"] += 1; seen["b"] += b; seen["r"] += r; seen["p"] += p; seen["q"] += p & b
            size = 12 + 8 * b
            if p:
                assert x > 0 and src is not None and not src["kind"].endswith("+r") and (src["kind"] == "both") == bool(b)
                out.append(dict(src, x=x, y=y, repeat=True))
                continue
            flags = wire[pos]
            src = dict(x=x, y=y, kind=("both" if b else "l1" if flags & MBCF_LIST1 else "l0") + ("+r" if r else ""), repeat=False, pos=pos,
                       head=wire[pos:pos + size], slice=wire[pos + 3], mbkind=P.MB_INTER)
            out.append(src)
            pos += size + 12 * r
    assert (seen["c"], seen["b"], seen["r"], seen["p"], seen["q"]) == (nc, nb, nr, np_, nq)
    assert pos - ent == eb == 32 * wm * hm - 20 * nc + 8 * nb + 12 * nr - 12 * np_ - 8 * nq
    return out


def at(ents, wm, x, y):
    return ents[y * wm + x]


def check_round_trip(name, pkt):
    """fold at level 3, unfold, refold: the wire bytes come back and the expansion is that of level 2"""
    wire = backend.packet_fold(pkt, 3)
    assert wire[4] == 7
    assert backend.packet_check(wire) == 0, (name, backend.last_error())
    back = backend.packet_expand(wire)
    assert backend.packet_check(back) == 0, (name, backend.last_error())
    assert backend.packet_fold(back, 3) == wire, name  # the expansion is canonical
    w2 = backend.packet_compact(pkt, level=2)
    assert back == backend.packet_expand(w2), name
    assert P.Packet(wire).mbs.tobytes() == P.Packet(back).mbs.tobytes()  # P.Packet reads a version-7 packet through its expansion
    return wire


def test_fold_unfold_refold():
    n = 0
    for name, pkt in all_packets():
        assert backend.packet_check(pkt) == 0
        check_round_trip(name, pkt)
        for level in (1, 2):  # the new entry point at the old levels: the old bytes
            assert backend.packet_fold(pkt, level) == backend.packet_compact(pkt, level=level), (name, level)
        n += 1
    assert n >= 13 + 16
    for level in (0, 4, -1):
        with pytest.raises(backend.BackendError, match="level"):
            backend.packet_fold(all_packets()[1][1], level)
    with pytest.raises(backend.BackendError, match="level"):
        backend.packet_compact(all_packets()[1][1], level=3)  # (the older entry point keeps its two levels)


def test_the_planted_runs_are_found():
    """every shape of tests/run_cases.py: the census of entry kinds and runs it is there for"""
    seen = {}
    for name, ft, pkt, ops in planted():
        wire = backend.packet_fold(pkt, 3)
        ents = entries(wire)
        wm = layout(wire)[0]
        reps = {(e["x"], e["y"]) for e in ents if e["repeat"]}
        want = run_cases.expected_repeats(ops, wm)
        assert want <= reps, (name, sorted(want - reps))
        assert not any(x == 0 for x, _ in reps), name
        for e in ents:
            if e["repeat"]:
                k = "repeat_" + e["kind"]
                seen[k] = seen.get(k, 0) + 1
        case = name.split("/")[0]
        if case == "1x1":
            assert not reps and len(wire) == len(backend.packet_compact(pkt, level=2)) + 16  # 8 bytes of header, one bitmap word, padding to 8
        if case == "33x3" and ft == "P":
            assert {(30, 0), (31, 0), (32, 0)} <= reps and at(ents, wm, 32, 0)["pos"] == at(ents, wm, 29, 0)["pos"]  # across the word boundary, to the row's end
            first = at(ents, wm, 0, 1)
            assert not first["repeat"] and first["head"] == at(ents, wm, 32, 0)["head"]  # equal to the last of the row above: its own bytes all the same
            assert (1, 1) in reps
            seen["row_start_equal"] = 1
        if case == "65x2" and ft in "PB":
            assert all((x, 0) in reps for x in range(21, 65)) and (20, 0) not in reps  # word 1 is all repeats ...
            assert at(ents, wm, 64, 0)["pos"] == at(ents, wm, 20, 0)["pos"]           # ... and the source of the row's last lies two words back
            assert all((x, 1) in reps for x in range(2 if ft == "P" else 1, 65))      # the whole row
            seen["two_words_back"] = 1
    # the 20x6 pictures: where the tail, the full record and the one-list / two-list pair were put
    for name, ft, pkt, ops in planted():
        if not name.startswith("20x6") or ft == "I":
            continue
        wire = backend.packet_fold(pkt, 3)
        ents, wm = entries(wire), layout(wire)[0]
        reps = {(e["x"], e["y"]) for e in ents if e["repeat"]}
        seen["slices"] = seen.get("slices", set()) | {e["slice"] for e in ents if e["repeat"]}
        for op, y, x, *rest in ops:
            if op == "tail":
                t, left, right = at(ents, wm, x, y), at(ents, wm, x - 1, y), at(ents, wm, x + 1, y)
                assert t["kind"].endswith("+r") and not t["repeat"]
                assert t["head"][1:] == left["head"][1:] and t["head"][0] & 0x0e == left["head"][0]  # the same head (but for T8x8 / LEV8 of its residual) ...
                assert left["repeat"] and not right["repeat"] and right["head"] == left["head"]     # ... cuts the run: its right neighbour has bytes again
                assert (x + 2, y) in reps
                seen["cut_by_tail"] = seen.get("cut_by_tail", 0) + 1
            if op == "full":
                f, left, right = at(ents, wm, x, y), at(ents, wm, x - 1, y), at(ents, wm, x + 1, y)
                assert f["kind"] == "full" and left["repeat"] and not right["repeat"] and right["head"] == left["head"] and (x + 2, y) in reps
                seen["cut_by_full"] = seen.get("cut_by_full", 0) + 1
            if op == "l0_of":
                one, two = at(ents, wm, x, y), at(ents, wm, x + 1, y)
                assert one["kind"] == "l0" and two["kind"] == "both" and not two["repeat"] and two["head"][:12] == one["head"] and (x + 2, y) in reps
                seen["l0_then_both"] = seen.get("l0_then_both", 0) + 1
    for k in ("repeat_l0", "repeat_l1", "repeat_both", "row_start_equal", "two_words_back", "cut_by_tail", "cut_by_full", "l0_then_both"):
        assert seen.get(k, 0) > 0, (k, seen)
    assert len(seen["slices"]) >= 3, seen
    assert seen["repeat_l0"] > 100 and seen["repeat_l1"] > 50 and seen["repeat_both"] > 50, seen


def test_the_expansion_decodes_to_the_same_pictures():
    """the oracle (a version-4 reader) on the planted packets and on their level-3 fold + unfold: same pictures"""
    for name, pics in run_cases.cases().items():
        w, h = run_cases.CASES[name][:2]
        nb = P.frame_bytes(w, h)
        rng = np.random.default_rng(1)
        dpb = [rng.integers(0, 256, nb + 16, dtype=np.uint8) for _ in range(6)] + [None] * 26
        dpb7 = [None if b is None else b.copy() for b in dpb]
        o4, o7 = Oracle(), Oracle()
        for ft, pkt, _ in pics:
            o4.decode_frame(pkt, dpb, 3)
            o7.decode_frame(backend.packet_expand(backend.packet_fold(pkt, 3)), dpb7, 3)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            assert np.array_equal(dpb[d][:nb], dpb7[d][:nb]), name


@needs_front
def test_every_committed_stream_folds_and_unfolds():
    saved = 0
    for f in sorted(glob.glob(os.path.join(STREAMS, "*.264"))):
        if os.path.getsize(f) > 400_000:
            continue
        for pkt in front.capture_packets(open(f, "rb").read())[0]:
            pkt = bytes(pkt)
            wire = check_round_trip(f, pkt)
            saved += len(backend.packet_compact(pkt, level=2)) - len(wire)
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
    """e264_expand.h run thread by thread on the host (it finds a repeat's source by arithmetic, e264_expand_mb by the search that defines it): the record
    array and the motion section it writes are the bytes of e264_expand_packet"""
    pe, _ = emu
    cases = wire_cases()
    assert len(cases) >= 29
    for name, wire in cases:
        _held_against_host_expansion(pe, name, wire, (256, 64 * 7, 1))


@needs_front
def test_expand_kernel_source_on_large_pictures(emu):
    """1080p packets of the encoder-shaped streams (120 x 68 macroblocks: four bitmap words per row), P and B pictures"""
    pe, _ = emu
    n = reps = 0
    for name in ("nat1080_ipp30.264", "cabac_nat1080_ibbp30.264"):
        pk = front.capture_packets(open(os.path.join(STREAMS, name), "rb").read())[0]
        for p in pk[1:8:3]:
            wire = check_round_trip(name, bytes(p))
            reps += int(np.frombuffer(wire, "<u4", 8, layout(wire)[3])[5])
            _held_against_host_expansion(pe, name, wire, (256, 64 * 7, 1))
            n += 1
    assert n == 6 and reps > 6000


def test_kernels_read_a_version7_packet_through_its_expansion(emu):
    """the four kernels' source on (version-7 packet + expansion buffer) against the same source on the version-4 packet: identical pictures and parameters"""
    pe, ie = emu
    n = 0
    for name, pics in run_cases.cases().items():
        w, h = run_cases.CASES[name][:2]
        nb = P.frame_bytes(w, h)
        rng = np.random.default_rng(7)
        dpb = [rng.integers(0, 256, nb + 64, dtype=np.uint8) for _ in range(6)] + [None] * 26
        for ft, pkt, _ in pics:
            wire = backend.packet_fold(pkt, 3)
            n += sum(1 for e in entries(wire) if e["repeat"])
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
            assert np.array_equal(res[0][0], res[1][0]), name
            assert np.array_equal(res[0][1], res[1][1]), name
            Oracle().decode_frame(pkt, dpb, 3)  # the next picture's references
    assert n > 400  # (repeats went through the kernels)


def test_damaged_version7_packets_are_refused_or_sound():
    """bytes of the header, the table, the bitmaps and the entries damaged at random: e264hip_packet_check either refuses the packet or its expansion is a
    sound version-4 packet (what the device unfolds is what was vetted)"""
    rng = np.random.default_rng(7)
    refused = accepted = 0
    for name, wire in wire_cases():
        wm, hm, wpr, base, _, bitmaps, ent = layout(wire)
        h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
        spans = ((0, int(h["payload_off"])), (base, ent), (bitmaps[3], ent))  # anywhere in front of the payload; the table; the repeat bitmap
        for k in range(120):
            buf = bytearray(wire)
            lo, hi = spans[k % 3]
            for _ in range(int(rng.integers(1, 4))):
                i = int(rng.integers(lo, hi))
                buf[i] = int(rng.integers(0, 256)) if rng.random() < 0.6 else buf[i] ^ (1 << int(rng.integers(0, 8)))
            buf = bytes(buf)
            if backend.packet_check(buf) != 0:
                refused += 1
                continue
            accepted += 1
            assert backend.packet_check(backend.packet_expand(buf)) == 0
    print(f"damaged version-7 packets: {refused} refused, {accepted} accepted")
    assert refused > 100 and accepted > 100


def _word(buf, off):
    return int.from_bytes(buf[off:off + 4], "little")


def _move_repeat(wire, y, set_x, clear_x):
    """pbits of row y with the bit of set_x set and that of clear_x cleared (both in one class of entries, so that every count of the header still agrees)"""
    wm, hm, wpr, base, _, bitmaps, ent = layout(wire)
    buf = bytearray(wire)
    for x, on in ((set_x, 1), (clear_x, 0)):
        o = bitmaps[3] + 4 * (y * wpr + (x >> 5))
        w = _word(buf, o)
        assert (w >> (x & 31) & 1) != on
        buf[o:o + 4] = (w ^ 1 << (x & 31)).to_bytes(4, "little")
    return bytes(buf)


def test_each_structure_rule_and_the_canonical_rule_broken_by_hand():
    pics = {f"{ft}{i}": p for i, (ft, p, _) in enumerate(run_cases.cases()["20x6"])}
    ops = {f"{ft}{i}": o for i, (ft, _, o) in enumerate(run_cases.cases()["20x6"])}
    wp, wb = backend.packet_fold(pics["P1"], 3), backend.packet_fold(pics["B2"], 3)
    assert backend.packet_check(wp) == 0 and backend.packet_check(wb) == 0
    t = next(x for op, y, x, *_ in ops["P1"] if op == "tail")

    def refused(buf, why):
        assert backend.packet_check(buf) != 0, why
        assert "structure" in backend.last_error(), (why, backend.last_error())
    # every move keeps n_repeat, n_repeat_both and entries_bytes what they are: the rule named is the one that refuses
    refused(_move_repeat(wp, 3, 10, 12), "pbits outside cbits: the full record as a repeat")
    refused(_move_repeat(wp, 2, t, t + 2), "pbits inside rbits: the tail entry as a repeat")
    refused(_move_repeat(wp, 1, 0, 1), "bit 0 of a row")
    refused(_move_repeat(wp, 3, 11, 12), "the left neighbour of a repeat is a full record")
    refused(_move_repeat(wp, 2, t + 1, t + 2), "the left neighbour of a repeat carries a tail")
    refused(_move_repeat(wb, 4, 6, 7), "the left neighbour of a repeat has one list, the repeat two")
    wm, hm, wpr, base, row_off, bitmaps, ent = layout(wp)
    for off, why in ((base + 20, "n_repeat"), (base + 24, "n_repeat_both"), (base + 28, "zero"), (base + 8, "entries_bytes"), (row_off + 8, "row_off"),
                     (bitmaps[3] + 4 * (5 * wpr), "a repeat more than counted")):
        bad = bytearray(wp)
        bad[off] ^= 1
        refused(bytes(bad), why)
    # canonical form: a plain entry with bytes of its own that equals the plain entry to its left should have been a repeat
    ents = entries(wp)
    pair = next((a, b) for a, b in zip(ents, ents[1:]) if a["y"] == b["y"] and a["kind"] == b["kind"] == "l0" and not a["repeat"] and not b["repeat"])
    bad = bytearray(wp)
    bad[pair[1]["pos"]:pair[1]["pos"] + 12] = pair[0]["head"]
    assert backend.packet_check(bytes(bad)) != 0 and "canonical" in backend.last_error()
    bad[pair[1]["pos"] + 8] ^= 1  # (one bit of the vector apart: sound again)
    assert backend.packet_check(bytes(bad)) == 0, backend.last_error()
    # ... also behind a repeat: the entry that ends a run by differing may not be made equal to it
    run_end = next(b for a, b in zip(ents, ents[1:]) if a["y"] == b["y"] and a["repeat"] and a["kind"] == b["kind"] == "l0" and not b["repeat"])
    bad = bytearray(wp)
    bad[run_end["pos"]:run_end["pos"] + 12] = at(ents, wm, run_end["x"] - 1, run_end["y"])["head"]
    assert backend.packet_check(bytes(bad)) != 0 and "canonical" in backend.last_error()


def test_wrong_form_inputs_are_refused():
    wire = backend.packet_fold(run_cases.cases()["20x6"][1][1], 3)
    assert backend.packet_check(wire) == 0
    assert backend.packet_check(wire[:-8]) != 0
    assert backend.packet_check(wire[:100]) != 0
    for v in (6, 5, 4):  # a version-7 packet relabelled
        other = bytearray(wire)
        other[4] = v
        assert backend.packet_check(bytes(other)) != 0, v
    for v, level in ((5, 1), (6, 2)):  # and the other way round
        other = bytearray(backend.packet_fold(run_cases.cases()["20x6"][1][1], level))
        assert other[4] == v
        other[4] = 7
        assert backend.packet_check(bytes(other)) != 0, v
    for level in (1, 2, 3):
        with pytest.raises(backend.BackendError):
            backend.packet_fold(wire, level)  # already folded
    with pytest.raises(backend.BackendError):
        backend.packet_expand(backend.packet_expand(wire))  # not a wire packet


@needs_front
def test_front_end_emits_the_same_version7_packets():
    """e264front_set_compact(3): what leaves the front end is the level-3 fold of what it would have sent (pictures without inter macroblocks leave as version 4)"""
    n7 = n4 = 0
    for f in SMALL:
        data = open(f, "rb").read()
        plain = [bytes(p) for p in front.capture_packets(data)[0]]
        wire = [bytes(p) for p in front.capture_packets(data, compact=3)[0]]
        assert len(plain) == len(wire), f
        for a, b in zip(plain, wire):
            assert backend.packet_check(b) == 0
            if b[4] == 7:
                assert b == backend.packet_fold(a, 3), f
                n7 += 1
            else:
                assert a == b and int(P.Packet(a).hdr["n_inter_mbs"]) == 0, f
                n4 += 1
    front.capture_packets(b"", compact=False)  # (the switch is global to the library: leave it off)
    assert n7 > 50 and n4 > 0


@needs_front
def test_front_end_folds_pictures_that_leave_in_several_packets():
    """ten damaged streams (a slice cut short and sent again: the picture goes out in several packets whose records are edited in the packet before they are
    folded): packet by packet the level-3 fold of what the front end sends with the option off"""
    from tests import damage
    n7 = multi = 0
    for c in damage.RESENT[:10]:
        data = damage.truncated_then_resent(*c)
        plain = [bytes(p) for p in front.capture_packets(data)[0]]
        wire = [bytes(p) for p in front.capture_packets(data, compact=3)[0]]
        assert len(plain) == len(wire)
        seen = {}
        for a, b in zip(plain, wire):
            assert backend.packet_check(b) == 0
            fid = int(P.Packet(a).hdr["frame_id"])
            seen[fid] = seen.get(fid, 0) + 1
            if b[4] == 7:
                assert b == backend.packet_fold(a, 3)
                n7 += 1
            else:
                assert a == b
        multi += sum(1 for v in seen.values() if v > 1)
    front.capture_packets(b"", compact=False)
    assert n7 > 20 and multi > 5


@needs_front
@pytest.mark.parametrize("name", FIXTURES_1080)
def test_sizes_on_the_1080p_fixtures(name):
    """level 3 is never larger than level 2; on the encoder-shaped streams it is below 0.57 of version 4 (counted on the fixtures before the level was
    built: 0.558 and 0.559 with the new bitmap, plus 8 bytes of header per picture, and a point of room)"""
    pk = [bytes(p) for p in front.capture_packets(open(os.path.join(STREAMS, name), "rb").read())[0]]
    b4 = b6 = b7 = 0
    for p in pk:
        w6, w7 = backend.packet_compact(p, level=2), backend.packet_fold(p, 3)
        b4, b6, b7 = b4 + len(p), b6 + len(w6), b7 + len(w7)
    print(f"{name}: v6/v4 {b6 / b4:.4f}  v7/v4 {b7 / b4:.4f}  ({b4} {b6} {b7} bytes, {len(pk)} packets)")
    assert b7 <= b6
    if name in ("nat1080_ipp30.264", "cabac_nat1080_ibbp30.264"):
        assert b7 < 0.57 * b4
