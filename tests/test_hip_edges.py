"""The kernels on the MI355X against the oracle at the ends of the weight, scaling, level and vector ranges (tests/edge_cases.py): weight
denominators 0..7 with the default weight 128 of denominator 7 and the (a & b) == 128 pairs, weights / offsets -128 / 127, scaling entries up
to 255 at QP 48..51 (the int16 wrap of the 8x8 dequantisation), int16 and byte-form level ends, vectors at +-32768 quarter samples, indexA /
indexB clamped at 0 and 51 around I_PCM.  tests/test_oracle_vs_refkernels.py pins the oracle to the reference's own kernels on the same
cases, tests/test_*_emu.py the kernels' source built for the host; here the device build meets them.  Every test also asserts that its
packets hold the edge it is named after."""
from collections import Counter

import pytest

from edge264_amd import backend, packet as P, synth
from tests import edge_cases
from tests.test_hip_forms import GEOMS, REACHES, SETTINGS, decoders, options, run_batch
from tests.test_hip_parity import run_stream

pytestmark = pytest.mark.gpu
W, H = 6, 5
CASES = edge_cases.CASES
MATRIX = [c for c in CASES if c[0] in ("denom7_and128", "scaling8_qp48_inter", "level_ends_inter", "level_ends_intra", "level_ends_qp51_dc")]


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def packets_of(w, h, seed, pattern, kw):
    """the packets run_stream submits for these arguments (the generator is seeded), checked by the validator"""
    pkts = synth.StreamSynth(w, h, seed, **kw).gop(pattern)
    for p in pkts:
        assert backend.packet_check(p) == 0
    return pkts


def assert_edges(seen, must, label):
    assert all(seen[k] for k in must), f"{label}: the packets miss an edge: {dict((k, seen[k]) for k in must)}"


@pytest.mark.parametrize("split", [True, False], ids=["passes_split", "submit"])
@pytest.mark.parametrize("name,pattern,kw,must", CASES, ids=[c[0] for c in CASES])
def test_edges_match_oracle(device, oracle, name, pattern, kw, must, split):
    seen = Counter()
    for seed in range(4):
        seen.update(edge_cases.stream_census(packets_of(W, H, seed, pattern, kw)))
        run_stream(device, oracle, seed, pattern, kw, W, H, passes_split=split)
    assert_edges(seen, must, name)


@pytest.mark.parametrize("how", ["host", "resident"])
@pytest.mark.parametrize("name,pattern,kw,must", CASES, ids=[c[0] for c in CASES])
def test_edges_in_wire_form(device, oracle, name, pattern, kw, must, how):
    """the same packets folded to the wire form (version 5, include/edge264_compact.h), three streams per submission"""
    gens = [synth.StreamSynth(w, h, 300 + k, **kw) for k, (w, h) in enumerate(GEOMS)]
    seen, folded = Counter(), 0
    with options(device) as cfg, decoders(device, len(gens)) as decs:
        for i, t in enumerate(pattern):
            v4s = [bytes(g.next_frame(t)) for g in gens]
            wire = [backend.packet_compact(p) for p in v4s]
            for p, wp in zip(v4s, wire):
                c = edge_cases.census(p)
                assert backend.packet_check(wp) == 0 and edge_cases.census(wp) == c  # (the edges survive the folding)
                seen.update(c)
            folded += sum(wp[4] == P.E264_VERSION_COMPACT for wp in wire)
            run_batch(device, oracle, how, decs, v4s, cfg, sent=wire, label=f"{name} wire frame {i}{t}")
    assert folded > 0
    assert_edges(seen, must, name)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name,pattern,kw,must", MATRIX, ids=[c[0] for c in MATRIX])
def test_edges_on_every_form(device, oracle, setting, name, pattern, kw, must):
    """test_hip_forms' feature matrix (deblocking / intra wave counts, side queue, two-workgroup and planes forms) on the weighted, scaling and
    level cases"""
    gens = [synth.StreamSynth(w, h, 700 + 13 * k, **kw) for k, (w, h) in enumerate(GEOMS)]
    total, seen = Counter(), Counter()
    with options(device, **SETTINGS[setting]) as cfg, decoders(device, len(gens)) as decs:
        for i, t in enumerate(pattern):
            pkts = [bytes(g.next_frame(t)) for g in gens]
            for p in pkts:
                seen.update(edge_cases.census(p))
            total.update(run_batch(device, oracle, "resident", decs, pkts, cfg, label=f"{name} {setting} frame {i}{t}"))
    assert sum(total[f] for f in REACHES[setting]) > 0, total
    assert_edges(seen, must, name)


def test_1080p_vectors_and_denominator_7(device, oracle):
    """120 x 68 macroblocks, I P B: vectors at the int16 ends (the edge-emulation clamp thousands of samples outside a wide picture) and
    explicit weights at denominator 7"""
    kw = dict(mv_ends=0.05, weighted=1, weight_denoms=[(7, 7)], weight_pins=0.3, t8x8=True, i_kinds=edge_cases.ALL_I)
    seen = edge_cases.stream_census(packets_of(120, 68, 23, "IPB", kw))
    assert_edges(seen, ["mv_ends", "denom7_default", "bipred_and128", "default_beside_explicit", "offset_ends"], "1080p")
    run_stream(device, oracle, 23, "IPB", kw, 120, 68, passes_split=False)
