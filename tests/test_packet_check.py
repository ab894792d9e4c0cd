"""e264hip_packet_check (include/edge264_hip.h): the host-side validation every host-packet entry point runs
before a packet may reach the device.  Host-only, so it is tested on the CPU: packets from the synthesiser and
from the reference front end (all fixtures) pass; each corruption a kernel would dereference is EINVAL, the
reference's error convention (positive errno, README.md:188-209), never a fault.
"""
import errno
import glob
import os
from collections import Counter

import numpy as np
import pytest

from edge264_amd import backend, packet as P, synth
from tests import edge_cases, layouts

HERE = os.path.dirname(os.path.abspath(__file__))
STREAMS = os.path.join(HERE, "golden", "streams")
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref")


@pytest.fixture(scope="module")
def gop():
    return synth.StreamSynth(6, 4, seed=11, num_refs=2).gop("IPB")


def test_synth_packets_pass(gop):
    for raw in gop:
        assert backend.packet_check(raw) == 0


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(REF), "..", "edge264_amd", "libedge264_hipfront.so")), reason="front end not built")
def test_front_end_packets_pass(oracle):
    from oracle.pyoracle import HipFront
    n = 0
    for path in sorted(glob.glob(os.path.join(STREAMS, "*.264"))):
        if "1080" in path:
            continue
        _, _, packets = HipFront().decode_capture(open(path, "rb").read(), oracle)
        for raw in packets:
            assert backend.packet_check(raw) == 0, os.path.basename(path)
            n += 1
    assert n > 40


def mutate(raw, fn):
    buf = bytearray(raw)
    pk = P.Packet(buf)   # numpy views over the bytearray are writable
    fn(pk, buf)
    return bytes(buf)


def first(pk, kind):
    return int(np.nonzero(pk.mbs["kind"] == kind)[0][0])


def hdr_set(field, value):
    def fn(pk, buf):
        h = np.frombuffer(buf, P.FRAME_HDR, 1)
        h[field] = value
    return fn


def mb_set(field, value, kind=None):
    def fn(pk, buf):
        mbs = np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))
        a = 7 if kind is None else first(pk, kind)
        mbs[field][a] = value
    return fn


def motion_set(byte, value):
    """Overwrite one byte of the first inter macroblock's compact motion record (version 3: byte 0 = refPic and byte 1 = refIdx
    of its first predicted part)."""
    def fn(pk, buf):
        a = first(pk, P.MB_INTER)
        mbs = np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))
        off = int(mbs["modes"][a][:4].view("<u4")[0])
        buf[int(pk.hdr["motion_off"]) + off + byte] = value & 255
    return fn


def directory_set(word, value):
    def fn(pk, buf):
        a = first(pk, P.MB_INTER)
        mbs = np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))
        mbs["modes"][a][word * 4:word * 4 + 4] = np.frombuffer(np.uint32(value).tobytes(), np.uint8)
    return fn


CORRUPTIONS = [
    ("magic", 0, hdr_set("magic", 0x12345678)),
    ("version", 0, hdr_set("version", 99)),
    ("total_bytes", 0, hdr_set("total_bytes", 1 << 30)),
    ("dst_slot", 0, hdr_set("dst_slot", 32)),
    ("dst_slot_neg", 0, hdr_set("dst_slot", -1)),
    ("zero_width", 0, hdr_set("width_mbs", 0)),
    ("huge_frame", 0, hdr_set("height_mbs", 4000)),
    ("mbs_off", 0, hdr_set("mbs_off", 1 << 28)),
    ("payload_off", 0, hdr_set("payload_off", 1 << 28)),
    ("payload_bytes", 0, hdr_set("payload_bytes", 1 << 28)),
    ("motion_off", 1, hdr_set("motion_off", 1 << 28)),
    ("motion_missing", 1, hdr_set("motion_off", 0)),
    ("n_slices", 0, hdr_set("n_slices", 1 << 20)),
    ("no_slices", 0, hdr_set("n_slices", 0)),
    ("stride_small", 0, hdr_set("stride_Y", 16)),
    ("plane_small", 0, hdr_set("plane_size_Y", 64)),
    ("kind", 0, mb_set("kind", 9)),
    ("slice_index", 0, mb_set("slice", 5)),
    ("mb_payload_off", 0, mb_set("payload_off", 1 << 27)),
    ("mb_payload_align", 0, mb_set("payload_off", 4)),
    ("coded_overrun", 0, mb_set("payload_off", None)),     # filled in below: last 8 bytes of the payload
    ("t8x8_on_i16x16", 0, None),                            # filled in below
    ("absent_wild_slice", 0, None),                         # filled in below: ABSENT records are read by the parameter kernel too
    ("refPic", 1, motion_set(0, 40)),
    ("refPic_neg", 1, motion_set(0, -3)),
    ("refPic_none", 1, motion_set(0, -1)),                  # a part the directory announces must name a picture
    ("refIdx", 1, motion_set(1, 77)),
    ("mot_off_align", 1, directory_set(0, 2)),
    ("mot_off_overrun", 1, directory_set(0, 1 << 26)),
    ("mot_hdr_bits", 1, directory_set(1, 1 << 27)),
]


@pytest.mark.parametrize("name,frame,fn", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_corruption_is_einval(gop, name, frame, fn):
    raw = gop[frame]
    if name == "coded_overrun":
        def fn(pk, buf):
            mbs = np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))
            a = int(np.nonzero(mbs["coded"] != 0)[0][0])
            mbs["payload_off"][a] = (int(pk.hdr["payload_bytes"]) - 8) & ~7
    if name == "t8x8_on_i16x16":
        def fn(pk, buf):
            mbs = np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))
            mbs["flags"][first(pk, P.MB_I16x16)] |= P.MBF_T8x8
    if name == "absent_wild_slice":
        def fn(pk, buf):
            mbs = np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))
            mbs["kind"][3] = P.MB_ABSENT
            mbs["slice"][3] = 60000
    bad = mutate(raw, fn)
    assert bad != raw
    assert backend.packet_check(bad) == errno.EINVAL
    assert backend.last_error()


def test_truncated_packet(gop):
    for cut in (0, 16, 79, 80, len(gop[1]) // 2, len(gop[1]) - 1):
        assert backend.packet_check(gop[1][:cut]) == errno.EINVAL


def test_byte_fuzz_never_faults(gop):
    """Random byte flips in the header / record sections: any verdict is fine, a crash is not."""
    rng = np.random.default_rng(3)
    raw = gop[2]
    pk = P.Packet(raw)
    limit = int(pk.hdr["payload_off"])
    for _ in range(300):
        buf = bytearray(raw)
        for _ in range(int(rng.integers(1, 6))):
            buf[int(rng.integers(0, limit))] = int(rng.integers(0, 256))
        assert backend.packet_check(bytes(buf)) in (0, errno.EINVAL)


@pytest.mark.parametrize("name,pattern,kw,must", edge_cases.CASES, ids=[c[0] for c in edge_cases.CASES])
def test_range_end_packets_pass(name, pattern, kw, must):
    """packets at the ends of the weight, scaling, level and vector ranges (tests/edge_cases.py) are legal: the validator accepts them in both
    forms, they hold the edge they are named after, and the wire form carries it unchanged"""
    seen = Counter()
    for seed in range(2):
        for raw in synth.StreamSynth(6, 5, seed, **kw).gop(pattern):
            c = edge_cases.census(raw)
            wire = backend.packet_compact(raw)
            assert backend.packet_check(raw) == 0 and backend.packet_check(wire) == 0
            assert edge_cases.census(wire) == c
            seen.update(c)
    assert all(seen[k] for k in must), {k: seen[k] for k in must}


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(REF), "..", "edge264_amd", "libedge264_hipfront.so")), reason="front end not built")
@pytest.mark.parametrize("name", ["weighted_denom7", "cabac_weighted_denom7"])
def test_denominator_7_fixtures_reach_the_edges(oracle, name):
    """the pred_weight_table fixtures at the ends of their ranges, through the real front end: denominator 7 with its default weight 128 in use,
    the (a & b) == 128 pairs, a default beside an explicit weight, weights and offsets -128 / 127, in P and B slices"""
    from oracle.pyoracle import HipFront
    _, _, packets = HipFront().decode_capture(open(os.path.join(STREAMS, name + ".264"), "rb").read(), oracle)
    seen = edge_cases.stream_census(packets)
    assert all(seen[k] for k in ("luma_denom7", "chroma_denom7", "denom7_default", "bipred_and128", "default_beside_explicit", "offset_ends",
                                 "weight_ends")), seen
    types = {int(s["slice_type"]) for p in packets for s in P.Packet(p).slices if s["luma_log2_weight_denom"] == 7}
    assert {0, 1} <= types, types


# ---- the layouts the gate accepts (include/edge264_cmd.h, E264FrameHdr.stride_Y .. plane_size_C) ---------------------------------------------

def _geom(raw, over):
    """raw with its four layout fields set to the tight layout's updated by over(tight header fields)"""
    g = layouts.hdr_of(raw)
    g.update(over(g))
    buf = bytearray(raw)
    h = np.frombuffer(buf, P.FRAME_HDR, 1)
    for k in ("stride_Y", "stride_C", "plane_size_Y", "plane_size_C"):
        h[k] = g[k]
    return bytes(buf)


def _rows(g):
    return g["height_mbs"] * 16


LAYOUT_BAD = [
    ("psY_plus4", lambda g: dict(plane_size_Y=g["stride_Y"] * _rows(g) + 4)),   # every chroma row 4 bytes off the alignment of stride_C
    ("psY_plus8", lambda g: dict(plane_size_Y=g["stride_Y"] * _rows(g) + 8)),
    ("psY_plus1", lambda g: dict(plane_size_Y=g["stride_Y"] * _rows(g) + 1)),
    ("psY_short", lambda g: dict(plane_size_Y=g["stride_Y"] * _rows(g) - 16)),
    ("psC_short", lambda g: dict(plane_size_C=g["stride_C"] * _rows(g) // 2 - 8)),
    ("stride_Y_plus8", lambda g: dict(stride_Y=g["stride_Y"] + 8, plane_size_Y=1 << 20)),
    ("stride_C_plus4", lambda g: dict(stride_C=g["stride_C"] + 4, plane_size_C=1 << 20)),
    ("stride_C_small", lambda g: dict(stride_C=g["width_mbs"] * 16 - 8)),
    ("frame_2GiB", lambda g: dict(plane_size_C=(1 << 31) - g["plane_size_Y"])),  # plane_size_Y + plane_size_C = 2^31: the kernels' offsets are 32-bit
    ("frame_8GiB", lambda g: dict(plane_size_Y=(1 << 32) - 16, plane_size_C=(1 << 32) - 8)),
]
LAYOUT_GOOD = [
    *[(f"layout_{k}", lambda g, k=k: layouts.geometry(g["width_mbs"], g["height_mbs"], k)) for k in layouts.LAYOUTS],
    ("psY_plus16", lambda g: dict(plane_size_Y=g["stride_Y"] * _rows(g) + 16)),
    ("psC_plus1", lambda g: dict(plane_size_C=g["stride_C"] * _rows(g) // 2 + 1)),  # (nothing lies behind chroma: its size needs no alignment)
    ("frame_below_2GiB", lambda g: dict(plane_size_C=(1 << 31) - 1 - g["plane_size_Y"])),
]


@pytest.mark.parametrize("form", ["version4", "wire"])
@pytest.mark.parametrize("name,over", LAYOUT_BAD, ids=[c[0] for c in LAYOUT_BAD])
def test_layout_refused(gop, name, over, form):
    for raw in gop:
        raw = backend.packet_compact(raw) if form == "wire" else raw
        bad = _geom(raw, over)
        assert bad != raw
        assert backend.packet_check(bad) == errno.EINVAL, name
        assert backend.last_error()


@pytest.mark.parametrize("form", ["version4", "wire"])
@pytest.mark.parametrize("name,over", LAYOUT_GOOD, ids=[c[0] for c in LAYOUT_GOOD])
def test_layout_accepted(gop, name, over, form):
    for raw in gop:
        raw = backend.packet_compact(raw) if form == "wire" else raw
        assert backend.packet_check(_geom(raw, over)) == 0, (name, backend.last_error())


@pytest.mark.parametrize("form", ["version4", "wire"])
def test_restride_keeps_every_other_byte(gop, form):
    """tests/layouts.py restride: the four layout fields change, nothing else; a wire packet keeps its form"""
    for raw in gop:
        raw = backend.packet_compact(raw) if form == "wire" else raw
        for k, lay in layouts.LAYOUTS.items():
            out = layouts.restride(raw, *lay)
            assert len(out) == len(raw) and out[4] == raw[4]
            diff = np.nonzero(np.frombuffer(out, np.uint8) != np.frombuffer(raw, np.uint8))[0]
            assert set(diff.tolist()) <= set(range(16, 32)), (k, diff)
            assert layouts.hdr_of(out) == dict(layouts.hdr_of(raw), **layouts.geometry(*P.Packet(raw).hdr[["width_mbs", "height_mbs"]].item(), k))
