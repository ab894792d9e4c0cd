"""The kernels on the MI355X on the pictures of tests/content_cases.py: sample values that take the reference's int16 vectors over their ends in
the 2-D six-tap (centre6r of e264_pred.h, classes 4 and 5), in the 8x8 inverse transform and in the DC-only add, the weighted sums to the
negative end of int16, and the deblocking filters through every decision the oracle counts.  tests/test_oracle_vs_refkernels.py holds the oracle
to the reference's own kernels on the same pictures and tests/test_*_emu.py the kernels' source built for the host; here the device build meets
them.  The expectation is the oracle's picture, and every test takes the census of that same oracle decode (Oracle.events()) and holds it to the
case's events: it proves its own reach without asking the code under test."""
import contextlib
from collections import Counter

import pytest

from edge264_amd import backend, synth
from tests import content_cases as cc
from tests.test_hip_forms import GEOMS, HOWS, REACHES, SETTINGS, decoders, options, run_batch, submit
from tests.test_hip_layouts import ldecoders, run_layout_batch
from tests.test_hip_parity import run_stream

pytestmark = pytest.mark.gpu
MATRIX = ["hv_wrap", "hv_wrap_weighted", "idct8_wrap"]


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


@contextlib.contextmanager
def census(oracle, name, label):
    """the events of every oracle decode inside the block, held to the case's list when it ends"""
    with oracle.events() as seen:
        yield seen
    must = cc.BY_NAME[name][3]
    assert not cc.missing(seen, must), f"{label}: counted fewer than {cc.FLOOR} times: {cc.missing(seen, must)}"


@pytest.mark.parametrize("split", [True, False], ids=["passes_split", "submit"])
@pytest.mark.parametrize("name,w,h", cc.RUNS, ids=cc.RUN_IDS)
def test_content_matches_oracle(device, oracle, name, w, h, split):
    with census(oracle, name, f"{name} {w}x{h}"):
        run_stream(device, oracle, cc.SEED, cc.pattern_of(name, w, h), cc.options_of(name), w, h, passes_split=split)


def three_streams(name):
    return [synth.StreamSynth(w, h, 700 + 13 * k, **cc.options_of(name)) for k, (w, h) in enumerate(GEOMS)]


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", MATRIX)
def test_content_in_batches(device, oracle, name, how):
    """three streams of different geometries per submission through every batch entry point"""
    gens = three_streams(name)
    with census(oracle, name, f"{name} {how}"), options(device) as cfg, decoders(device, len(gens)) as decs:
        for i, t in enumerate(cc.BY_NAME[name][1]):
            run_batch(device, oracle, how, decs, [bytes(g.next_frame(t)) for g in gens], cfg, label=f"{name} frame {i}{t}")


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", MATRIX)
def test_content_on_every_form(device, oracle, setting, name):
    """test_hip_forms' settings (deblocking / intra wave counts, side queue, two-workgroup and planes forms)"""
    gens = three_streams(name)
    total = Counter()
    with census(oracle, name, f"{name} {setting}"), options(device, **SETTINGS[setting]) as cfg, decoders(device, len(gens)) as decs:
        for i, t in enumerate(cc.BY_NAME[name][1]):
            total.update(run_batch(device, oracle, "resident", decs, [bytes(g.next_frame(t)) for g in gens], cfg, label=f"{name} {setting} frame {i}{t}"))
    assert sum(total[f] for f in REACHES[setting]) > 0, total


def test_hv_wrap_in_wire_form_level_3(device, oracle):
    """the same packets folded to version 7 (include/edge264_compact.h), submitted as host packets: the expansion kernel in front"""
    w, h = 6, 5
    name = "hv_wrap"
    with census(oracle, name, "wire form level 3"), decoders(device, 1) as decs:
        for i, p in enumerate(cc.packets(name, w, h)):
            wire = backend.packet_fold(bytes(p), 3)
            assert wire[4] == 7 and backend.packet_check(wire) == 0
            decs[0].prepare(bytes(p))
            submit(device, "host", decs, [wire])
            decs[0].check(oracle, bytes(p), f"{name} wire form level 3, picture {i}")


@pytest.mark.parametrize("layout", ["pad16", "gaps_wide"])
def test_hv_wrap_on_padded_layouts(device, oracle, layout):
    """padding right of every row and gaps behind the planes (tests/layouts.py): the samples are the oracle's, every other byte of every slot
    stays as it was uploaded (run_layout_batch)"""
    w, h = 6, 5
    name = "hv_wrap"
    with census(oracle, name, layout), options(device) as cfg, ldecoders(device, [layout], seed=4) as decs:
        for i, p in enumerate(cc.packets(name, w, h)):
            run_layout_batch(device, oracle, "host", decs, [bytes(p)], cfg, label=f"{name} picture {i}")
