"""The kernels' source built for the host (tests/emu) against the oracle on padded picture layouts (tests/layouts.py): padding right of
every row, gaps behind the planes, a narrow picture in a wide canvas.  Each picture goes through the whole pipeline of a submission --
the expansion of a wire packet, the parameter kernel (both forms), the prediction kernel, the intra kernel (scan, bitmap and planes forms)
and the deblocking kernel (mixed waves, luma and chroma waves; both builds) -- and then:
- its samples equal the oracle's;
- every other byte of the destination slot (padding, gaps, guard) is as it was;
- every byte of every other slot is as it was.
The oracle's slots hold other random bytes outside the samples than the kernels' do, so an output that depends on a byte that is not a
sample differs too.  No layout reaches the device before it passes here (and under AddressSanitizer, tests/test_frontend_sanitized.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, packet as P, synth
from oracle.pyoracle import Oracle, _dpb_array
from tests import edge_cases, layouts as L

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_I = (P.MB_I4x4, P.MB_I8x8, P.MB_I16x16)
N_SLOTS = 7  # the synthesiser's 6 slots and one no packet names


@pytest.fixture(scope="module")
def libs():
    d = os.path.join(HERE, "emu")
    subprocess.run(["make", "-C", d], check=True, stdout=subprocess.DEVNULL)
    out = {k: C.CDLL(os.path.join(d, f)) for k, f in (("product", "libe264_pred_emu.so"), ("gs2", "libe264_pred_emu_gs2.so"), ("intra", "libe264_intra_emu.so"))}
    for lib in out.values():
        for fn in ("e264emu_pred_frame2", "e264emu_intra_frame2"):
            if hasattr(lib, fn):
                getattr(lib, fn).argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        if hasattr(lib, "e264emu_expand"):
            lib.e264emu_expand.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
            lib.e264emu_deblock_frame2.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
            lib.e264emu_dbkparam_frame2.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
            lib.e264emu_dbkparam_frame2_nol1.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        lib.e264emu_set_expand.argtypes = [C.c_void_p]
    out["intra"].e264emu_intra_frame_planes.argtypes = [C.c_char_p, C.c_void_p]
    return out


# (deblocking build, intra form, deblocking waves, packet form): every build, form and wave kind meets every layout
VARIANTS = {
    "product_scan_mixed_v4": ("product", "scan", 0, "v4"),
    "product_bitmap_split_wire": ("product", "bitmap", 1, "wire"),
    "gs2_planes_split_v4": ("gs2", "planes", 1, "v4"),
    "gs2_bitmap_mixed_wire": ("gs2", "bitmap", 0, "wire"),
}


def has_l1(v4):
    pk = P.Packet(v4)
    inter = pk.mbs["kind"] == P.MB_INTER
    return bool(inter.any() and (pk.motion["refPic"][inter, 4:] >= 0).any())


def run_pipeline(libs, variant, v4, dpb):
    """one picture through the kernels' source, in the order of a submission on the device"""
    build, intra, split, form = VARIANTS[variant]
    pe, ie = libs[build], libs["intra"]
    h = L.hdr_of(v4)
    n = h["width_mbs"] * h["height_mbs"]
    pkt, area = v4, None
    if form == "wire":
        pkt = backend.packet_compact(v4)
        x = P.Packet(backend.packet_expand(pkt)).hdr
        area = np.full(int(x["payload_off"]) - int(x["mbs_off"]), 0xA5, np.uint8)
        assert pe.e264emu_expand(pkt, area.ctypes.data, 256) == 0
    for lib in (pe, ie):
        lib.e264emu_set_expand(None if area is None else area.ctypes.data)
    try:
        scratch = np.full(n * 146 + 64, 0x5A, np.uint8)  # E264_SCRATCH_BYTES (e264_kernels.h), stale
        prm = pe.e264emu_dbkparam_frame2 if has_l1(v4) else pe.e264emu_dbkparam_frame2_nol1  # (the launcher's choice)
        assert prm(pkt, scratch.ctypes.data, None) == 0
        arr = _dpb_array(dpb)
        if intra == "bitmap":
            assert pe.e264emu_pred_frame2(pkt, arr, scratch.ctypes.data) == 0
            assert ie.e264emu_intra_frame2(pkt, arr, scratch.ctypes.data) == 0
        else:
            assert pe.e264emu_pred_frame2(pkt, arr, None) == 0
            assert (ie.e264emu_intra_frame_planes(pkt, arr) if intra == "planes" else ie.e264emu_intra_frame2(pkt, arr, None)) == 0
        assert pe.e264emu_deblock_frame2(pkt, arr, scratch.ctypes.data, split) == 0
    finally:
        for lib in (pe, ie):
            lib.e264emu_set_expand(None)


def lose_macroblocks(raw, rng):
    """a lost slice: a run of macroblocks E264_MB_ABSENT (they keep their samples, include/edge264_cmd.h)"""
    buf = bytearray(raw)
    pk = P.Packet(buf)
    n = len(pk.mbs)
    mbs = np.frombuffer(buf, P.MB, n, int(pk.hdr["mbs_off"]))
    a = int(rng.integers(0, max(1, n - 3)))
    mbs["kind"][a:a + int(rng.integers(1, 2 * pk.width_mbs + 1))] = P.MB_ABSENT
    P.refresh_summary(buf)
    return bytes(buf)


def check_slots(hdr, before, after, label):
    """the destination changes in its samples at most; every other slot not at all"""
    d = hdr["dst_slot"]
    m = L.sample_mask(hdr)
    for s, (b, a) in enumerate(zip(before, after)):
        if b is None:
            continue
        keep = ~m if s == d else np.ones(len(b), bool)
        if not np.array_equal(a[keep], b[keep]):
            want = a.copy()
            want[keep] = b[keep]
            raise AssertionError(L.first_difference(hdr, a, want, f"{label}: slot {s}" + (" (destination, outside its samples)" if s == d else " (not the destination)")))


def run_case(libs, variant, layout, w, h, pattern, kw, seed, absent=False, oracle=None, name="", packets=None):
    """packets: the stream's tight packets, where the caller has generated them already (pattern, kw and seed then only label the run)"""
    g = synth.StreamSynth(w, h, seed, **kw) if packets is None else None
    rng = np.random.default_rng(seed + 17)
    oracle = oracle or Oracle()
    mine = theirs = None
    for i, t in enumerate(pattern):
        raw = bytes(g.next_frame(t) if packets is None else packets[i])
        if absent and i:
            raw = lose_macroblocks(raw, rng)
        v4 = L.in_layout(raw, layout)
        hdr = L.hdr_of(v4)
        if mine is None:  # random pictures to start from, the same samples on both sides, other bytes outside them
            mine = [L.random_slot(hdr, rng) for _ in range(N_SLOTS)] + [None] * (P.MAX_SLOTS - N_SLOTS)
            theirs = [None if a is None else L.random_slot(hdr, rng, samples_from=a) for a in mine]
        label = f"{name} {variant} {layout} {w}x{h} seed {seed} frame {i}{t}"
        before = [None if a is None else a.copy() for a in mine]
        before_o = [None if a is None else a.copy() for a in theirs]
        run_pipeline(libs, variant, v4, mine)
        oracle.decode_frame(v4, theirs, 3)
        check_slots(hdr, before, mine, label)
        check_slots(hdr, before_o, theirs, label + " (the oracle)")
        d = hdr["dst_slot"]
        for k, (a, b) in enumerate(zip(L.samples(hdr, mine[d]), L.samples(hdr, theirs[d]))):
            bad = a != b
            assert not bad.any(), f"{label}: {('luma', 'chroma [Cb | Cr]')[k]} differs from the oracle at (y, x) {np.argwhere(bad)[:5].tolist()}"
        # new random bytes outside the samples of some slots on the kernels' side: no output may depend on them
        for s in range(N_SLOTS):
            if not rng.integers(0, 3):
                mine[s] = L.random_slot(hdr, rng, samples_from=mine[s])


CASES = [
    ("ipbb", 5, 4, "IPBB", dict(num_refs=2)),
    ("t8x8_pcm_slices_idc2", 6, 5, "IPB", dict(t8x8=True, pcm_prob=0.2, slices_per_frame=3, deblock_idc=2, i_kinds=ALL_I, scaling=True)),
    ("explicit_far_mvs", 4, 3, "IPBP", dict(weighted=1, stress=True, mv_range=400, residual_prob=0.8)),
    ("intra_in_inter", 7, 6, "IPP", dict(intra_in_inter=0.4, filter_offsets=(-6, 6), i_kinds=ALL_I)),
    ("uni_tiles_b_weighted", 18, 3, "IPBB", dict(p_skip=0.95, weighted=1)),
    ("implicit_pskip", 7, 5, "IPBB", dict(p_skip=0.6, weighted=2)),
    ("one_mb", 1, 1, "IPB", dict(t8x8=True, i_kinds=ALL_I, mv_range=100)),
    ("one_by_four", 1, 4, "IPB", dict(mv_range=100)),
    ("five_by_one", 5, 1, "IPB", dict(mv_range=100, pcm_prob=0.1)),
]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", list(L.LAYOUTS))
def test_layouts_emu_vs_oracle(libs, oracle, layout, variant):
    for k, (name, w, h, pattern, kw) in enumerate(CASES):
        run_case(libs, variant, layout, w, h, pattern, kw, seed=31 * k + 5, oracle=oracle, name=name)


@pytest.mark.parametrize("variant", ["product_scan_mixed_v4", "gs2_bitmap_mixed_wire"])
@pytest.mark.parametrize("layout", L.PADDED)
def test_absent_macroblocks_keep_their_samples(libs, oracle, layout, variant):
    for seed in (1, 2):
        run_case(libs, variant, layout, 9, 6, "IPBP", dict(t8x8=True, i_kinds=ALL_I), seed, absent=True, oracle=oracle, name="absent")


EDGES = [c for c in edge_cases.CASES if c[0] in ("denom7_and128", "scaling8_qp48_inter", "level_ends_inter", "level_ends_intra", "mv_ends",
                                                  "filter_qp51")]


@pytest.mark.parametrize("name,pattern,kw,must", EDGES, ids=[c[0] for c in EDGES])
def test_range_ends_on_layouts(libs, oracle, name, pattern, kw, must):
    """the cases of tests/edge_cases.py, each on a padded layout and through another variant"""
    for k, layout in enumerate(L.PADDED[:3]):
        run_case(libs, list(VARIANTS)[(k + len(name)) % len(VARIANTS)], layout, 6, 5, pattern, kw, seed=k, oracle=oracle, name=name)
