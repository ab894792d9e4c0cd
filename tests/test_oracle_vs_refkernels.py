"""Differential pin of the oracle against the REFERENCE'S OWN static kernels
(oracle/_ref/libe264_refkernels.so = /root/reference/src/edge264_{intra,inter,residual,deblock}.c
behind oracle/ref_kernels_harness.c) on seeded synthetic packets.  Covers what the
reference has no in-repo golden vector for: dequant + 4x4/8x8 IDCT,
DC transforms, weighted prediction (explicit / implicit / default), edge emulation,
bS derivation and the deblocking filters, scaling lists, multi-slice edges.
Skipped where oracle/_ref is not built (it travels prebuilt to the GPU box)."""
import numpy as np
import pytest

from edge264_amd import packet as P
from edge264_amd import synth
from tests import content_cases, edge_cases, layouts, split_cases, structure_cases

W, H = 6, 5
ALL_I = (P.MB_I8x8, P.MB_I4x4, P.MB_I16x16)
CASES = [
    ("intra4x4_16x16", "IIII", dict()),
    ("intra8x8", "III", dict(i_kinds=ALL_I, t8x8=True)),
    ("pcm", "II", dict(pcm_prob=0.2)),
    ("scaling_lists", "II", dict(scaling=True, i_kinds=ALL_I)),
    ("ippp", "IPPPP", dict()),
    ("ippp_t8x8_scaling", "IPPPP", dict(t8x8=True, scaling=True)),
    ("ippp_explicit_wp", "IPPPP", dict(weighted=1)),
    ("ibbp", "IPBBPBB", dict()),
    ("ibbp_explicit_wp", "IPBBPBB", dict(weighted=1, t8x8=True)),
    ("ibbp_implicit_wp", "IPBBPBB", dict(weighted=2, t8x8=True, scaling=True)),
    ("slices_idc2", "IPBBP", dict(slices_per_frame=4, deblock_idc=2)),
    ("slices_idc0", "IPBBP", dict(slices_per_frame=4, deblock_idc=0)),
    ("filter_offsets", "IPB", dict(filter_offsets=(6, -4))),
    ("filter_offsets_neg", "IPB", dict(filter_offsets=(-10, 8), qp_base=36)),
    ("no_deblock", "IPB", dict(deblock=False)),
    ("stress_explicit", "IPBBP", dict(stress=True, weighted=1, t8x8=True, scaling=True, i_kinds=ALL_I)),
    ("stress_implicit_far_mv", "IPBBP", dict(stress=True, weighted=2, t8x8=True, mv_range=400)),
]


def run_stream(oracle, refkernels, seed, pattern, kw, w=W, h=H, seen=None, layout=None):
    """layout (a name of tests/layouts.py LAYOUTS): the packets restrided, slots of the layout's size plus a guard, other random bytes outside
    the samples on the two sides; the samples must agree and no other byte of any slot may change"""
    s = synth.StreamSynth(w, h, seed, **kw)
    nb = P.frame_bytes(w, h) + 16
    rng = np.random.default_rng(seed + 1000)
    ns = kw.get("n_slots", 6)
    if layout is None:
        dpb_o = [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(ns)] + [None] * (32 - ns)
        dpb_r = [a.copy() if a is not None else None for a in dpb_o]
    else:
        hdr = layouts.geometry(w, h, layout)
        hdr.update(width_mbs=w, height_mbs=h)
        dpb_o = [layouts.random_slot(hdr, rng) for _ in range(ns)] + [None] * (32 - ns)
        dpb_r = [layouts.random_slot(hdr, rng, samples_from=a) if a is not None else None for a in dpb_o]
        keep_o = [a.copy() if a is not None else None for a in dpb_o]
        keep_r = [a.copy() if a is not None else None for a in dpb_r]
        m = layouts.sample_mask(hdr)
    for i, t in enumerate(pattern):
        pkt = s.next_frame(t)
        if layout is not None:
            pkt = layouts.in_layout(pkt, layout)
        d = int(P.Packet(pkt).hdr["dst_slot"])
        if seen is not None:
            seen.update(edge_cases.census(pkt))
        for passes in (1, 2):  # reconstruction, then deblocking: compared after each
            oracle.decode_frame(pkt, dpb_o, passes)
            refkernels.replay(pkt, dpb_r, w, h, passes)
            if layout is None:
                assert np.array_equal(dpb_o[d], dpb_r[d]), f"seed {seed} frame {i}{t} pass {passes}"
                continue
            assert np.array_equal(dpb_o[d][m], dpb_r[d][m]), f"{layout} seed {seed} frame {i}{t} pass {passes}: samples differ"
            for side, dpb, keep in (("oracle", dpb_o, keep_o), ("reference", dpb_r, keep_r)):
                for k in range(ns):
                    same = dpb[k] == keep[k]
                    assert same[~m].all() if k == d else same.all(), \
                        layouts.first_difference(hdr, dpb[k], np.where(m if k == d else False, dpb[k], keep[k]), f"{layout} seed {seed} frame {i}{t} pass {passes}: {side} slot {k}")
        if layout is not None:
            keep_o[d][:], keep_r[d][:] = dpb_o[d], dpb_r[d]


@pytest.mark.parametrize("name,pattern,kw", CASES, ids=[c[0] for c in CASES])
def test_oracle_matches_reference_kernels(oracle, refkernels, name, pattern, kw):
    for seed in range(4):
        run_stream(oracle, refkernels, seed, pattern, kw)


def test_qp_range(oracle, refkernels):
    """The oracle against the reference kernels over the whole QP range (every qP % 6 / qP / 6 dequantiser case of both
    transforms with custom scaling lists, both ends of the alpha / beta / tC0 tables): the GPU test of the same name
    compares the kernels with the oracle."""
    for qp in range(0, 52, 3):
        run_stream(oracle, refkernels, 60 + qp, "IPB", dict(qp_base=qp, t8x8=True, scaling=True, i_kinds=ALL_I, residual_prob=0.8), 4, 3)


def test_many_references(oracle, refkernels):
    """16 references per list (17 slots), explicit and implicit weights indexed up to refIdx 15."""
    run_stream(oracle, refkernels, 51, "IPPPPPPPPPPPPPPPPBPB", dict(num_refs=16, n_slots=17, weighted=1, i_kinds=ALL_I, t8x8=True), 5, 4)
    run_stream(oracle, refkernels, 52, "IPPPPPPPPPPPPPPPPBPB", dict(num_refs=16, n_slots=17, weighted=2), 5, 4)


def test_per_slice_tables(oracle, refkernels):
    """Six slices per picture, each with its own scaling lists and weight tables."""
    for seed in range(3):
        run_stream(oracle, refkernels, seed, "IPBBP", dict(slices_per_frame=6, weighted=1, scaling=True, t8x8=True, i_kinds=ALL_I))
        run_stream(oracle, refkernels, seed, "IPBBP", dict(slices_per_frame=6, weighted=2, scaling=True, t8x8=True, i_kinds=ALL_I))


def test_max_frame_size(oracle, refkernels):
    """4096 x 2304 (256 x 144 macroblocks, the level 5.1/5.2 maximum; padded chroma stride): oracle vs reference kernels;
    the GPU test of the same name compares the kernels with the oracle on the same picture size."""
    run_stream(oracle, refkernels, 31, "IP", dict(t8x8=True, i_kinds=ALL_I), 256, 144)


def test_odd_geometry(oracle, refkernels):
    """1-MB-wide / 1-MB-high frames: every neighbour unavailable somewhere, all MC clamps."""
    # The reference's edge test `(unsigned)yInt_Y - yWide*2 >= height - h + 1 - yWide*5`
    # (src/edge264_inter.c:1203-1204) goes negative -> huge unsigned when a 16-high (wide) partition meets
    # a 16-sample-high (wide) frame with a fractional vector, so edge emulation is skipped and the reference
    # reads outside the frame.  Degenerate geometry only; the harness issues 4x4 calls here, which are exact.
    refkernels.lib.ref_force_4x4_calls(1)
    try:
        for (w, h) in ((1, 1), (1, 4), (5, 1), (2, 2)):
            run_stream(oracle, refkernels, 7, "IPB", dict(t8x8=True, i_kinds=ALL_I, mv_range=100), w, h)
    finally:
        refkernels.lib.ref_force_4x4_calls(0)


@pytest.mark.parametrize("name,pattern,kw,must", edge_cases.CASES, ids=[c[0] for c in edge_cases.CASES])
def test_range_ends(oracle, refkernels, name, pattern, kw, must):
    """The values at the ends of what a packet may carry (tests/edge_cases.py): weight denominators 0..7, the default weight 128 of
    denominator 7 and the (a & b) == 128 pairs, weights / offsets -128 / 127, scaling entries up to 255 at QP 48..51, int16 and byte-form
    level ends, vectors at +-32768, indexA / indexB clamped by offsets of +-12 at QP 0 and 51 around I_PCM."""
    from collections import Counter
    seen = Counter()
    for seed in range(4):
        run_stream(oracle, refkernels, seed, pattern, kw, seen=seen)
    assert all(seen[k] for k in must), {k: seen[k] for k in must}


@pytest.mark.parametrize("name,w,h", content_cases.RUNS, ids=content_cases.RUN_IDS)
def test_content_cases(oracle, refkernels, name, w, h):
    """The pictures of tests/content_cases.py, whose sample values take the reference's int16 vectors over their ends (the 2-D six-tap, the 8x8
    transform, the DC-only add) and its saturating weighted sums to the negative end: the one place where the oracle's model of those wraps is
    held to the reference's own kernels.  The census of the same decode must hold the case's events."""
    with oracle.events() as seen:
        run_stream(oracle, refkernels, content_cases.SEED, content_cases.pattern_of(name, w, h), content_cases.options_of(name), w, h)
    must = content_cases.BY_NAME[name][3]
    assert not content_cases.missing(seen, must), content_cases.missing(seen, must)


def test_range_ends_wide(oracle, refkernels):
    """Vectors at the int16 ends on a picture 1920 samples wide, weights at denominator 7: the edge-emulation clamp far from both sides."""
    from collections import Counter
    seen = Counter()
    run_stream(oracle, refkernels, 9, "IPBP", dict(mv_ends=0.3, weighted=1, weight_denoms=[(7, 7)], weight_pins=0.3, t8x8=True,
                                                    i_kinds=ALL_I), 120, 3, seen=seen)
    assert seen["mv_ends"] and seen["denom7_default"] and seen["bipred_and128"], seen


STRUCTURE = [(c[0], w, h) for c in structure_cases.SATURATED for (w, h) in c[1]]


@pytest.mark.parametrize("name,w,h", STRUCTURE, ids=[f"{n}_{w}x{h}" for n, w, h in STRUCTURE])
def test_saturated_structure(oracle, refkernels, name, w, h):
    """The pictures of tests/structure_cases.py that fill a tile's class lists and residual lists (1024 4x4 partitions of one interpolation
    class, every block of every macroblock coded): the oracle stays pinned to the reference's kernels where the kernel tests lean on it."""
    _, _, pattern, kw, _ = structure_cases.CASES[name]
    structure_cases.check(name, w, h)  # (the packets run_stream makes from the same seed and options: their census)
    run_stream(oracle, refkernels, structure_cases.seed_of(name, w, h), pattern, kw, w, h)


SPLIT = [(shape, w, h) for shape in split_cases.SHAPES for (w, h) in ((6, 5), (17, 5))]


@pytest.mark.parametrize("shape,w,h", SPLIT, ids=[f"{s}_{w}x{h}" for s, w, h in SPLIT])
def test_split_pictures(oracle, refkernels, shape, w, h):
    """Pictures sent in several packets (tests/split_cases.py: E264_MBF_DONE records beside fresh ones, macroblocks deblocked by a later packet than the
    one that reconstructed them), the rich stream, its census held against the shape's minimum: compared after every packet's reconstruction pass and
    again after its deblocking.  A DONE I_PCM record has no payload: a harness that copied one from payload offset 0 would overwrite what the
    earlier packet finished."""
    from tests.test_hip_parity import describe_mismatch
    pkts, labels = split_cases.flat(split_cases.packets(shape, "rich", w, h))
    nb = P.frame_bytes(w, h)
    rng = np.random.default_rng(w + h)
    dpb_o = [rng.integers(0, 256, nb + 16, dtype=np.uint8) for _ in range(6)] + [None] * 26
    dpb_r = [a.copy() if a is not None else None for a in dpb_o]
    for pkt, label in zip(pkts, labels):
        d = int(P.Packet(pkt).hdr["dst_slot"])
        for passes in (1, 2):
            oracle.decode_frame(pkt, dpb_o, passes)
            refkernels.replay(pkt, dpb_r, w, h, passes)
            assert np.array_equal(dpb_o[d], dpb_r[d]), f"{shape} {w}x{h} packet {label} pass {passes}, oracle / reference kernels: " + \
                describe_mismatch(P.Packet(pkt), dpb_o[d][:nb], dpb_r[d][:nb], w, h)


LAYOUT_CASES = [c for c in CASES if c[0] in ("intra8x8", "pcm", "ibbp_explicit_wp", "ibbp_implicit_wp", "slices_idc2", "stress_implicit_far_mv")]


# The reference's edge emulation finds the last row of a plane from its size (src/edge264_inter.c:1212, :1225: plane_size_Y - stride_Y), so
# it holds only where no gap follows a plane -- as in every layout it makes itself.  The oracle and the kernels take it from height_mbs.
REF_LAYOUTS = [k for k, (_, _, gap_y, gap_c) in layouts.LAYOUTS.items() if not gap_y and not gap_c]


@pytest.mark.parametrize("layout", REF_LAYOUTS)
def test_layouts_match_reference_kernels(oracle, refkernels, layout):
    """The oracle, the judge of every kernel test, against the reference's own kernels on pictures with padding right of every row
    (tests/layouts.py; luma rows and the chroma base 16-byte aligned, as in the reference's own frames): both honour the strides and
    plane_size_Y alike, and neither writes a byte outside the samples."""
    for k, (name, pattern, kw) in enumerate(LAYOUT_CASES):
        run_stream(oracle, refkernels, 200 + k, pattern, kw, layout=layout)
    edge = [c for c in edge_cases.CASES if c[0] in ("denom7_and128", "level_ends_inter", "mv_ends", "filter_qp51")]
    for k, (name, pattern, kw, _) in enumerate(edge):
        run_stream(oracle, refkernels, 300 + k, pattern, kw, layout=layout)
    refkernels.lib.ref_force_4x4_calls(1)  # (the odd geometries: see test_odd_geometry)
    try:
        for (w, h) in ((1, 1), (1, 4), (5, 1)):
            run_stream(oracle, refkernels, 7, "IPB", dict(t8x8=True, i_kinds=ALL_I, mv_range=100), w, h, layout=layout)
    finally:
        refkernels.lib.ref_force_4x4_calls(0)
