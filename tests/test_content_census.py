"""What the samples' values make the arithmetic do, counted by the oracle itself (oracle/e264_oracle.c E264O_EVENTS, Oracle.events()): the
census that holds tests/content_cases.py to the events its cases are named after, every event to a case, and the older case lists to the
deblocking decisions they have always reached.  CPU only: the counters are the oracle's, so a test that compares a kernel with the oracle on
a case knows from here what that comparison covered."""
from collections import Counter

import numpy as np
import pytest

from edge264_amd import packet as P, synth
from tests import content_cases as cc, edge_cases
from tests.test_oracle_vs_refkernels import CASES as PARITY_CASES

W, H = 6, 5
# every decision of the deblocking filters: tests/test_oracle_vs_refkernels.py CASES and tests/edge_cases.py CASES each reach all of them
DBK_PINNED = ["dbk_soft_ap_aq", "dbk_soft_ap", "dbk_soft_aq", "dbk_soft_none", "dbk_soft_delta_clip", "dbk_soft_clip255", "dbk_soft_p1_clip",
              "dbk_hard_both", "dbk_hard_p", "dbk_hard_q", "dbk_hard_not_small", "dbk_hard_small_none",
              "dbk_alpha_m1", "dbk_alpha", "dbk_beta_m1", "dbk_beta", "dbk_small_m1", "dbk_small",
              "dbkc_soft", "dbkc_soft_delta_clip", "dbkc_soft_clip255", "dbkc_hard"]


def list_census(oracle, cases, seeds):
    """census of (name, pattern, options) cases at 6 x 5 from the random slots the parity runners start from"""
    seen = Counter()
    with oracle.events() as got:
        for _, pattern, kw in cases:
            for seed in seeds:
                g = synth.StreamSynth(W, H, seed, **kw)
                dpb = cc.start_dpb(W, H, seed)
                for t in pattern:
                    oracle.decode_frame(g.next_frame(t), dpb, 3)
    seen.update(got)
    return seen


@pytest.fixture(scope="module")
def edge_census(oracle):
    return list_census(oracle, [c[:3] for c in edge_cases.CASES], range(4))


def test_names_are_a_fixed_list(oracle):
    names = oracle.event_names()
    assert len(names) == len(set(names)) >= 50 and set(DBK_PINNED) <= set(names)
    assert {e for c in cc.CASES for e in c[3]} <= set(names), "a case asks for an event the oracle does not count"
    with oracle.events() as seen:
        pass
    assert list(seen) == names and not any(seen.values())


@pytest.mark.parametrize("name,w,h", cc.RUNS, ids=cc.RUN_IDS)
def test_counting_changes_no_picture(oracle, name, w, h):
    """the same stream with the counters off: the pictures counted in content_cases.decode(), byte for byte (the guard behind them too)"""
    pkts, counted, _ = cc.decode(name, w, h)
    dpb = cc.start_dpb(w, h)
    for i, pkt in enumerate(pkts):
        oracle.decode_frame(pkt, dpb, 3)
        assert np.array_equal(dpb[int(P.Packet(pkt).hdr["dst_slot"])], counted[i]), f"{name} {w}x{h} picture {i}"
    with oracle.events() as seen:  # (and nothing was counted while they were off)
        pass
    assert not any(seen.values())


@pytest.mark.parametrize("name,w,h", cc.RUNS, ids=cc.RUN_IDS)
def test_case_reaches_its_events(name, w, h):
    seen = cc.decode(name, w, h)[2]
    assert not cc.missing(seen, cc.BY_NAME[name][3]), f"{name} {w}x{h}: counted fewer than {cc.FLOOR} times: {cc.missing(seen, cc.BY_NAME[name][3])}"


def test_every_event_has_a_case(oracle, edge_census):
    """an event no case of content_cases.CASES + edge_cases.CASES reaches is arithmetic the suite cannot see: adding an event forces a case"""
    seen = Counter(edge_census)
    for name, w, h in cc.RUNS:
        seen.update(cc.decode(name, w, h)[2])
    assert not [n for n in oracle.event_names() if not seen[n]]
    owned = {e for c in cc.CASES for e in c[3]}
    assert not [n for n in oracle.event_names() if n not in owned and edge_census[n] < cc.FLOOR], "an event without an owner must be dense in edge_cases"


def test_older_lists_keep_their_deblocking_reach(oracle, edge_census):
    """no count is pinned, only the set: a change to the generator that drops one of the filters' decisions from a list shows here"""
    parity = list_census(oracle, PARITY_CASES, (1, 2))
    assert not [n for n in DBK_PINNED if not parity[n]], "tests/test_oracle_vs_refkernels.py CASES"
    assert not [n for n in DBK_PINNED if not edge_census[n]], "tests/edge_cases.py CASES"
