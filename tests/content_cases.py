"""Pictures whose SAMPLE VALUES take the arithmetic where no draw of the generator's takes it: the int16 wrap of the 2-D six-tap, the wraps of the
8x8 inverse transform, the wrap of the DC-only add, the negative saturations of the weighted prediction, and every decision of the deblocking
filters.  tests/edge_cases.py counts from the packet that a case holds the edge it is named after; these cases are held to the oracle's event
counters (oracle/e264_oracle.c E264O_EVENTS, Oracle.events()): each must count every event of its `must` list at least FLOOR times at each of
its sizes, so a test that runs a case proves from the oracle's own decode -- not from the code under test -- that it reached the arithmetic.

The crafted samples arrive as I_PCM pictures (StreamSynth's pcm_samples), so a case is nothing but packets and goes through every runner and
entry point like any other.  An I_PCM macroblock has qP 0: its edges have alpha 0 and the deblocking leaves the samples as sent (decode()
asserts it on every picture made of I_PCM alone)."""
import functools
from collections import Counter

import numpy as np

from edge264_amd import packet as P, synth
from tests.edge_cases import FULL, NORM8

FLOOR = 16  # several lanes and positions meet the event, not one
SIZES = ((6, 5), (17, 5), (2, 2))  # 17: one macroblock more than a prediction tile's row; 2 x 2: every window leaves the picture
SEED = 5


def inter_everywhere(mbx, mby, w, h):
    return "inter"


# ---- the lattice: rows and columns of period 3, so that the six sums of a 2-D six-tap sit at (10710, -2550, 10710, 10710, -2550, 10710) ----

def lattice_mb(frame_no, mbx, mby):
    """Y[y][x] = 255 where (x % 3 != 1) == (y % 3 != 1), else 0, in picture coordinates; pictures of odd number hold the inverse.  There
    x2 = ((af - be) >> 2) + (cd - be) of the reference's sixtapHV leaves int16 on both sides."""
    y, x = np.mgrid[mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
    luma = np.where((x % 3 != 1) == (y % 3 != 1), 255, 0)
    y, x = np.mgrid[mby * 8:mby * 8 + 8, mbx * 8:mbx * 8 + 8]
    chroma = np.where((x % 3 != 1) == (y % 3 != 1), 255, 0)
    mb = np.concatenate([luma.ravel(), chroma.ravel(), 255 - chroma.ravel()]).astype(np.uint8)
    return (255 - mb if frame_no & 1 else mb).tobytes()


HV = dict(pcm_prob=1.0, pcm_samples=lattice_mb, place=inter_everywhere, mv_classes=(4, 5), num_refs=2, residual_prob=0.0, mv_range=16)
HV_ALL = ["hv_wrap_pos_c4", "hv_wrap_neg_c4", "hv_wrap_pos_c5", "hv_wrap_neg_c5", "hv_wrap_visible"]


# ---- 8x8 blocks whose vectors 0 and 4 sit at the same int16 end ----------------------------------------------------------------------------

class Idct8Ends:
    """level_hook: lanes 0..3 of vectors 0 and 4 of every 8x8 block dequantise to the same end of int16 (flat scaling lists), so that the first
    butterflies d0 + d4 of the first pass wrap; the ends alternate from block to block.  Below qP 36 the levels are +-32767 and the
    dequantisation saturates; from 36 on they are the largest whose product stays inside int16, and one more level of +-32767 wraps it."""

    def __init__(self):
        self.n = 0

    def __call__(self, what, qp):
        if what != "luma8x8":
            return None
        self.n += 1
        sign = 1 if self.n & 1 else -1
        c = np.zeros(64, np.int64)
        for pos in (0, 1, 2, 3, 32, 33, 34, 35):
            factor = 16 * int(NORM8[qp % 6][pos]) << max(qp // 6 - 6, 0)
            c[pos] = sign * (32767 if qp < 36 else 32767 // factor)
        if qp >= 36:
            c[9] = sign * 32767
        return c


# ---- DC-only blocks whose value sits just inside int16, over samples of 255 ------------------------------------------------------------------

_NA0 = (10, 11, 13, 14, 16, 18)  # normAdjust4x4 at position 0


def _dc_level(qp, chroma):
    """the largest level L <= 32767 (alone in its DC block, flat scaling lists) whose DC-only residual r = (dc + 32) >> 6 stays inside int16:
    a sample of 255 plus r then wraps wherever r > 32512 (transform_dc4x4 / transform_dc2x2 and add_dc4x4 of oracle/e264_oracle.c)"""
    ls = (16 * _NA0[qp % 6]) << (qp // 6)
    r = lambda L: ((((L * ls) >> 5) if chroma else ((L * ls + 32) >> 6)) + 32) >> 6  # noqa: E731
    L = min(32767, (32768 * 64 * (32 if chroma else 64)) // ls)
    while r(L) > 32767:
        L -= 1
    return L


class DcEnds:
    """level_hook: every luma and chroma DC block holds one level: by turns the one of _dc_level (the add wraps) and 32767 (from qP 30 on the
    DC-only residual leaves int16 and is truncated)"""

    def __init__(self):
        self.n = 0

    def __call__(self, what, qp):
        if what not in ("luma_dc", "chroma_dc"):
            return None
        self.n += 1
        c = np.zeros(16, np.int64)
        c[0] = _dc_level(qp, what == "chroma_dc") if self.n & 1 else 32767
        if what == "chroma_dc":
            c[1] = c[0]  # (Cb at the even positions, Cr at the odd ones)
        return c


def white_mb(frame_no, mbx, mby):
    return b"\xff" * 384


def thirds(mbx, mby, w, h):
    return ("pcm", "intra", "inter")[(mbx + mby) % 3]


# ---- smooth ramps: steps of a few levels, so that the differences the deblocking filters test sit around alpha, beta and tC ------------------

def ramp_mb(frame_no, mbx, mby):
    """Even macroblock rows: a slope of 3/4 of a level per sample folded into 0..255, with small seeded steps, in picture coordinates.  Odd rows:
    plateaus at 255 (rows 1, 5, ..) or 0 (rows 3, 7, ..) with notches of 5 levels a sample, period 7 so that a notch meets the edges at every
    offset: where a plateau ends one sample from an edge, p0 + delta of the bS < 4 filters leaves 0..255."""
    rng = np.random.default_rng((frame_no, mbx, mby))

    def plane(n, x0, y0, ax, ay):
        y, x = np.mgrid[y0:y0 + n, x0:x0 + n]
        if mby & 1:
            notch = np.array((0, 0, 0, 0, 5, 10, 5))[(x + y // 3 + frame_no) % 7]
            return (notch if mby & 2 else 255 - notch).ravel()
        v = np.abs(((x * ax + y * ay) // 4 + 60 * frame_no + 300) % 510 - 255)
        return np.clip(v + rng.integers(-2, 3, (n, n)), 0, 255).ravel()
    return np.concatenate([plane(16, mbx * 16, mby * 16, 3, -2), plane(8, mbx * 8, mby * 8, -3, 2), plane(8, mbx * 8, mby * 8, 2, 3)]).astype(np.uint8).tobytes()


class SmallSteps:
    """level_hook: one level of +-1 or +-2 at one of the three lowest frequencies of every block: residuals of a few grey levels, so that the
    pictures predicted from the ramps stay smooth and the steps at the block edges sit around the filters' thresholds"""

    def __init__(self):
        self.rng = np.random.default_rng(0)

    def __call__(self, what, qp):
        n = 64 if what == "luma8x8" else 16
        c = np.zeros(n, np.int64)
        pos = (0, 1, 8 if n == 64 else 4)[int(self.rng.integers(0, 3))] if what != "ac" else (1, 4)[int(self.rng.integers(0, 2))]
        c[pos] = (-2, -1, 1, 2)[int(self.rng.integers(0, 4))]
        return c


def some_intra(mbx, mby, w, h):
    """two macroblocks in five intra (never I_PCM, whose qP of 0 would switch the filter off at its edges), the others inter"""
    return "inter" if (2 * mbx + 3 * mby) % 5 > 1 else "intra"


DBK_ALL = ["dbk_soft_ap_aq", "dbk_soft_ap", "dbk_soft_aq", "dbk_soft_none", "dbk_soft_delta_clip", "dbk_soft_clip255", "dbk_soft_p1_clip",
           "dbk_hard_both", "dbk_hard_p", "dbk_hard_q", "dbk_hard_not_small", "dbk_hard_small_none",
           "dbk_alpha_m1", "dbk_alpha", "dbk_beta_m1", "dbk_beta", "dbk_small_m1", "dbk_small",
           "dbkc_soft", "dbkc_soft_delta_clip", "dbkc_soft_clip255", "dbkc_hard"]

# (name, picture types, generator options (callables: a case's stream is made by options_of(), which gives a stateful hook a fresh start),
#  events that must be counted FLOOR times, sizes)
CASES = [
    ("hv_wrap", "IIPBB", HV, HV_ALL, SIZES),
    ("hv_wrap_4x4", "IIPBB", dict(HV, partitions="4x4"), HV_ALL, SIZES),
    ("hv_wrap_weighted", "IIPBB", dict(HV, both_lists=True, weighted=1, **FULL), HV_ALL, SIZES),
    ("hv_wrap_far", "IIPBB", dict(HV, mv_range=400), HV_ALL, SIZES),
    ("hv_wrap_residual", "IIPBB", dict(HV, residual_prob=0.9, t8x8=True), HV_ALL, SIZES),
    ("hv_wrap_one_class_4", "IIPBB", dict(HV, mv_classes=(4,)), ["hv_wrap_pos_c4", "hv_wrap_neg_c4", "hv_wrap_visible"], SIZES),
    ("hv_wrap_one_class_5", "IIPBB", dict(HV, mv_classes=(5,)), ["hv_wrap_pos_c5", "hv_wrap_neg_c5", "hv_wrap_visible"], SIZES),
    ("idct8_wrap", "IPPIP", dict(t8x8=True, i_kinds=(P.MB_I8x8,), coded_all=True, qp_base=36, level_hook=Idct8Ends),
     ["idct8_wrap", "idct8_wrap_visible", "idct8_dequant_sat", "idct8_dequant_wrap"], SIZES),
    ("dc_add_wrap", "IPP", dict(pcm_prob=1.0, pcm_samples=white_mb, place=thirds, i_kinds=(P.MB_I16x16,), qp_base=40, residual_prob=1.0,
                                chroma_qp_offsets=(0, 0), level_hook=DcEnds),
     ["dc4_add_wrap", "dc4_trunc"], SIZES),
    ("wp_neg_sat", "IIBB", dict(pcm_prob=1.0, pcm_samples=white_mb, place=inter_everywhere, both_lists=True, weighted=1,
                                weight_range=(-128, -128), offset_range=(-128, -128), residual_prob=0.0),
     ["madd_sat_neg", "adds_sat_neg", "wp_pack_lo"], SIZES),
    ("smooth", "IPPPIPPP", dict(pcm_prob=1.0, pcm_samples=ramp_mb, place=some_intra, residual_prob=0.5, p_skip=0.5, mv_range=8, mv_classes=(0, 0, 1, 2), num_refs=2, qp_base=32,
                                level_hook=SmallSteps),
     DBK_ALL, SIZES),
]
BY_NAME = {c[0]: c for c in CASES}
RUNS = [(c[0], w, h) for c in CASES for (w, h) in c[4]]
RUN_IDS = [f"{n}_{w}x{h}" for n, w, h in RUNS]


def options_of(name):
    """the generator options of a case; a hook given as a class is made anew, so that every stream of the case starts it alike"""
    kw = dict(BY_NAME[name][2])
    if isinstance(kw.get("level_hook"), type):
        kw["level_hook"] = kw["level_hook"]()
    return kw


def pattern_of(name, w, h):
    """the case's picture types; a picture of four macroblocks or fewer holds too few samples, so there the pattern is sent ten times over
    (hv_wrap_far forty times: of its vectors of +-100 samples one in ten leaves a window any sample of a 32 x 32 picture)"""
    p = BY_NAME[name][1]
    return p * (40 if name == "hv_wrap_far" else 10) if w * h <= 4 else p


def packets(name, w, h, seed=SEED):
    return synth.StreamSynth(w, h, seed, **options_of(name)).gop(pattern_of(name, w, h))


def start_dpb(w, h, seed=SEED):
    """six slots of random bytes, as the runners of the parity tests start from"""
    rng = np.random.default_rng(seed + 1000)
    return [rng.integers(0, 256, P.frame_bytes(w, h) + 16, dtype=np.uint8) for _ in range(6)] + [None] * 26


def assert_pcm_intact(pkt, picture, label=""):
    """every I_PCM macroblock of a picture made of I_PCM alone holds, after deblocking, the samples the packet carries"""
    pk = P.Packet(bytes(pkt))
    if not (pk.mbs["kind"] == P.MB_PCM).all():
        return False
    w, h = pk.width_mbs, pk.height_mbs
    g = P.frame_geometry(w, h)
    luma = picture[:g["plane_size_Y"]].reshape(-1, g["stride_Y"])
    chroma = picture[g["plane_size_Y"]:g["plane_size_Y"] + g["plane_size_C"]].reshape(-1, g["stride_C"])
    for a, m in enumerate(pk.mbs):
        x, y = a % w, a // w
        o = pk.payload_off + int(m["payload_off"])
        sent = np.frombuffer(pk.data, np.uint8, 384, o)
        assert np.array_equal(luma[y * 16:y * 16 + 16, x * 16:x * 16 + 16].ravel(), sent[:256]), f"{label}: I_PCM luma of macroblock ({x}, {y}) filtered"
        for pl in range(2):
            c0 = pl * (g["stride_C"] // 2) + x * 8
            assert np.array_equal(chroma[y * 8:y * 8 + 8, c0:c0 + 8].ravel(), sent[256 + 64 * pl:320 + 64 * pl]), f"{label}: I_PCM chroma of macroblock ({x}, {y}) filtered"
    return True


@functools.lru_cache(maxsize=None)
def _decode(name, w, h):
    from oracle.pyoracle import Oracle
    orc = Oracle()
    pkts = packets(name, w, h)
    dpb = start_dpb(w, h)
    pictures, crafted = [], 0
    with orc.events() as seen:
        for i, pkt in enumerate(pkts):
            orc.decode_frame(pkt, dpb, 3)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            crafted += assert_pcm_intact(pkt, dpb[d], f"{name} {w}x{h} picture {i}")
            pictures.append(dpb[d].copy())
    assert crafted or "pcm_samples" not in BY_NAME[name][2], f"{name}: no picture of I_PCM alone"
    return pkts, pictures, seen


def decode(name, w, h):
    """(packets, the oracle's picture after each -- deblocked, from start_dpb() --, census of the whole stream): computed once per process and
    shared; treat all three as read-only"""
    pkts, pictures, seen = _decode(name, w, h)
    return pkts, pictures, Counter(seen)


def missing(seen, must):
    """the events of `must` counted fewer than FLOOR times, with their counts"""
    return {k: seen[k] for k in must if seen[k] < FLOOR}
