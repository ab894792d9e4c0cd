"""The kernels on the MI355X on padded picture layouts (tests/layouts.py): padding right of every row, gaps behind the planes, a narrow
picture in a wide canvas, and batches whose streams each have their own layout.

Every slot is allocated with plane_size_Y + plane_size_C and a guard behind, and filled with random bytes in full.  After every submission,
for every stream in it, every slot is downloaded whole:
- the destination's samples equal the oracle's;
- every other byte of the destination, and every byte of every other slot (the references and the slots the packet does not name), is what
  was uploaded.
Every submission runs twice: the second time the slots hold the same samples and other random bytes everywhere else, and the oracle's slots
a third pattern, so an output that depends on a byte that is not a sample fails.  Every submission's launch counts must be what the rule
table says (tests/test_hip_forms.py), so each form is counted on padded layouts.  tests/test_layouts_emu.py runs the same layouts through
the kernels' source on the host first."""
import contextlib
from collections import Counter

import numpy as np
import pytest

from edge264_amd import backend, packet as P, synth
from tests import edge_cases, layouts as L
from tests.test_hip_forms import (COMPOSITION, GEOMS, REACHES, SETTINGS, expected_submission, n_cus, observed, options, submit,
                                  tiny_gens)
from tests.test_layouts_emu import lose_macroblocks

pytestmark = pytest.mark.gpu
ALL_I = (P.MB_I4x4, P.MB_I8x8, P.MB_I16x16)
N_SLOTS = 7  # the synthesiser's 6 slots and one no packet names


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


class LDec:
    """one decoder whose slots are in one layout, on the device and on the oracle's side"""

    def __init__(self, dev, layout, seed, lane=0):
        self.st = backend.Stream(dev, 1, 1)
        if lane:
            self.st.bind_lane(lane)
        self.layout, self.lane = layout, lane
        self.rng = np.random.default_rng(seed)
        self.hdr = None
        self.truth = [None] * P.MAX_SLOTS  # the oracle's slots

    def prepare(self, v4):
        """on the first picture: N_SLOTS slots of the picture's layout plus the guard, random pictures to start from"""
        hdr = L.hdr_of(v4)
        geo = {k: hdr[k] for k in ("width_mbs", "height_mbs", "stride_Y", "stride_C", "plane_size_Y", "plane_size_C")}
        if self.hdr is None:
            self.hdr = geo
            self.st.frame_bytes = L.slot_bytes(geo)
            for s in range(N_SLOTS):
                self.st.alloc(s)
                self.truth[s] = L.random_slot(geo, self.rng)
        assert geo == self.hdr, "a stream keeps its layout"
        self.pkt_hdr = hdr

    def upload(self, before):
        """every slot in full: the samples of `before`, new random bytes everywhere else"""
        self.sent = [L.random_slot(self.hdr, self.rng, samples_from=before[s]) for s in range(N_SLOTS)]
        for s, img in enumerate(self.sent):
            self.st.upload(s, img)

    def check(self, label):
        h = self.pkt_hdr
        d = h["dst_slot"]
        m = L.sample_mask(h)
        for s in range(N_SLOTS):
            got = self.st.download(s)
            want = self.sent[s].copy()
            if s == d:
                want[m] = self.truth[d][m]
            if not np.array_equal(got, want):
                raise AssertionError(L.first_difference(h, got, want, f"{label}, layout {self.layout}: slot {s}" + (" (the destination)" if s == d else
                                                                                                                  " (not the destination)")))

    def close(self):
        self.st.close()


@contextlib.contextmanager
def ldecoders(dev, layouts, seed=0, lanes=(0,)):
    ds = []
    try:
        for k, lay in enumerate(layouts):
            ds.append(LDec(dev, lay, seed + k, lanes[k % len(lanes)]))
        yield ds
    finally:
        dev.sync()
        for d in ds:
            d.close()


def run_layout_batch(dev, oracle, how, decs, raws, cfg, wire=(), max_lane=0, label="", mode=None):
    """one submission of raws[k] (tight packets) restrided to decs[k]'s layout, twice, as described above; wire: the indices sent in wire
    form.  Returns the forms launched (counted once)."""
    v4s = [L.in_layout(p, d.layout) for d, p in zip(decs, raws)]
    sent = [L.in_layout(backend.packet_compact(p), d.layout) if k in wire else v4 for k, (d, p, v4) in enumerate(zip(decs, raws, v4s))]
    for d, p in zip(decs, v4s):
        d.prepare(p)
    before = [[None if a is None else a.copy() for a in d.truth] for d in decs]
    for d, p in zip(decs, v4s):
        oracle.decode_frame(p, d.truth, 3 if mode is None else mode)
    want = None if mode is not None else expected_submission(dev, how, v4s, sent, cfg, max_lane)
    for run in (1, 2):
        for d, b in zip(decs, before):
            d.upload(b)
        observed(dev)  # (reset)
        if mode is None:
            submit(dev, how, decs, sent)
        else:
            assert how == "host"
            dev.submit_batch_host([d.st for d in decs], sent, mode=mode)
        for k, d in enumerate(decs):
            d.check(f"{label} picture {k} of {len(decs)} ({how}, run {run})")
        got = observed(dev)
        if want is not None:
            assert got == want, f"{label} ({how}, run {run}): launched {got}, the rules say {want}"
    return got


# ---- every setting of the device, on two padded layouts ------------------------------------------------------------------------------------

RICH = dict(t8x8=True, pcm_prob=0.1, slices_per_frame=2, deblock_idc=2, weighted=1, num_refs=2, intra_in_inter=0.2, i_kinds=ALL_I)


@pytest.mark.parametrize("layout", ["pad16", "gaps_wide"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_settings_on_layouts(device, oracle, setting, layout):
    """three streams of different geometries, I_PCM, two slices with deblock_idc 2, weights, intra in P / B pictures, under every setting"""
    gens = [synth.StreamSynth(w, h, 40 + 7 * k, **RICH) for k, (w, h) in enumerate(GEOMS)]
    total = Counter()
    with options(device, **SETTINGS[setting]) as cfg, ldecoders(device, [layout] * len(gens), seed=len(setting)) as decs:
        for i, t in enumerate("IPBP"):
            total.update(run_layout_batch(device, oracle, "resident", decs, [bytes(g.next_frame(t)) for g in gens], cfg, label=f"{setting} frame {i}{t}"))
    assert sum(total[f] for f in REACHES[setting]) > 0, total


# ---- the rule boundaries, small pictures ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,how", [("canvas", "resident"), ("pad16", "host")])
def test_rule_boundaries_on_layouts(device, oracle, layout, how):
    """all-I batches (no prediction kernel) at 128 / 129 pictures, P-only batches (the small parameter kernel), split-off I pictures at
    48 / 49 and the others at 320 / 321 (on a 256-CU device)"""
    cus = n_cus(device)
    half, nn = cus // 2, cus * 3 // 16
    n = max(2 * half + 1, 322, nn + 101)
    gens = tiny_gens(n, 4000)
    with options(device) as cfg, ldecoders(device, [layout] * n, seed=9) as decs:
        def batch(ks, t, label):
            ks = list(ks)
            return run_layout_batch(device, oracle, how, [decs[k] for k in ks], [bytes(gens[k].next_frame(t)) for k in ks], cfg, label=label)

        def mixed(n_i, n_p, label):
            ks = range(n_i + n_p)
            return run_layout_batch(device, oracle, how, [decs[k] for k in ks], [bytes(gens[k].next_frame("I" if k < n_i else "P")) for k in ks], cfg, label=label)
        f = batch(range(half), "I", f"all-I n={half}")
        assert f["intra_planes_alone"] == half and f["dbk_planes"] == half and "pred" not in f, f
        f = batch(range(half, 2 * half + 1), "I", f"all-I n={half + 1}")
        assert f["intra16_nobitmap"] == half + 1 and f["dbk2_8"] == half + 1 and "intra_planes_alone" not in f, f
        batch(range(2 * half + 1, n), "I", "the other streams' first pictures")
        f = batch(range(half), "P", f"P n={half}")
        assert f["dbk_planes"] == half and f["dbkp_small"] == half, f
        f = batch(range(half + 1), "P", f"P n={half + 1}")
        assert f["dbk2_8"] == half + 1 and f["dbkp_small"] == half + 1, f
        f = mixed(nn, 100, f"mixed {nn} I + 100 P")
        assert f["intra_planes_split"] == nn, f
        f = mixed(nn + 1, 100, f"mixed {nn + 1} I + 100 P")
        assert f["intra_split"] == nn + 1 and "intra_planes_split" not in f, f
        f = mixed(1, 320, "mixed 1 I + 320 P")
        assert f["intra_planes_split"] == 1, f
        f = mixed(1, 321, "mixed 1 I + 321 P")
        assert f["intra_split"] == 1 and "intra_planes_split" not in f, f


# ---- every entry point, shapes 1x1 .. 120x68, version-4 and wire packets, each stream its own layout ---------------------------------------

@pytest.mark.parametrize("how", ["single", "resident", "host", "pinned", "pinned_untrusted"])
def test_entry_points_on_mixed_layouts(device, oracle, how):
    gens = [synth.StreamSynth(w, h, seed=950 + k, num_refs=2, t8x8=bool(k & 1), intra_in_inter=0.1, p_skip=0.6, pcm_prob=0.05)
            for k, ((w, h), _) in enumerate(COMPOSITION)]
    lays = [L.MIXED[k % len(L.MIXED)] for k in range(len(gens))]
    total = Counter()
    with options(device) as cfg, ldecoders(device, lays, seed=3) as decs:
        for i in range(len(COMPOSITION[0][1])):
            raws = [bytes(g.next_frame(gop[i])) for g, (_, gop) in zip(gens, COMPOSITION)]
            total.update(run_layout_batch(device, oracle, how, decs, raws, cfg, wire={k for k in range(len(raws)) if (k + i) & 1}, label=f"composition {i}"))
    assert total["dbkp_general"] > 0 and total["pred"] > 0, total
    if how != "resident":
        assert total["expand"] > 0, total


@pytest.mark.parametrize("name,pattern,kw,must", edge_cases.CASES, ids=[c[0] for c in edge_cases.CASES])
def test_range_ends_on_mixed_layouts(device, oracle, name, pattern, kw, must):
    """the cases of tests/edge_cases.py, three streams per submission, each in its own padded layout, the middle one in wire form"""
    gens = [synth.StreamSynth(w, h, 500 + k, **kw) for k, (w, h) in enumerate(GEOMS)]
    lays = [L.PADDED[(len(name) + k) % len(L.PADDED)] for k in range(len(gens))]
    with options(device) as cfg, ldecoders(device, lays, seed=len(name)) as decs:
        for i, t in enumerate(pattern):
            run_layout_batch(device, oracle, "host", decs, [bytes(g.next_frame(t)) for g in gens], cfg, wire={1}, label=f"{name} frame {i}{t}")


@pytest.mark.parametrize("layout", ["canvas", "gaps"])
def test_absent_macroblocks_on_layouts(device, oracle, layout):
    """lost slices (E264_MB_ABSENT) keep their samples, the last picture has nothing in it and leaves the slot as it was"""
    gens = [synth.StreamSynth(9, 6, 41 + k, t8x8=True, i_kinds=ALL_I) for k in range(2)]
    rng = np.random.default_rng(1)
    with options(device) as cfg, ldecoders(device, [layout] * 2, seed=5) as decs:
        for i, t in enumerate("IPBP"):
            raws = [bytes(g.next_frame(t)) for g in gens]
            raws = [lose_macroblocks(r, rng) if i else r for r in raws]
            if i == 3:
                buf = bytearray(raws[1])
                pk = P.Packet(buf)
                np.frombuffer(buf, P.MB, len(pk.mbs), int(pk.hdr["mbs_off"]))["kind"][:] = P.MB_ABSENT
                P.refresh_summary(buf)
                raws[1] = bytes(buf)
            run_layout_batch(device, oracle, "resident", decs, raws, cfg, label=f"absent frame {i}{t}")


def test_max_frame_on_padded_layout(device, oracle):
    """256 x 144 macroblocks (4096 x 2304, whose tight strides are already padded) with more padding and gaps"""
    g = synth.StreamSynth(256, 144, 31, t8x8=True, i_kinds=ALL_I)
    with options(device) as cfg, ldecoders(device, ["gaps_wide"], seed=2) as decs:
        for i, t in enumerate("IP"):
            run_layout_batch(device, oracle, "single", decs, [bytes(g.next_frame(t))], cfg, label=f"4096x2304 frame {i}{t}")


@pytest.mark.parametrize("layout", ["tight", "pad_wide"])
def test_baseline_config1_on_layouts(device, oracle, layout):
    """BASELINE.json configs[1] at its stated shape: 1080p (120 x 68 macroblocks) all-intra 4x4, every block coded, no deblocking, reconstruction
    only (RUN_RECON); three seeds"""
    gens = [synth.StreamSynth(120, 68, seed, i_kinds=(P.MB_I4x4,), residual_prob=1.0, deblock=False) for seed in range(3)]
    with options(device) as cfg, ldecoders(device, [layout] * len(gens), seed=11) as decs:
        for i in range(2):
            run_layout_batch(device, oracle, "host", decs, [bytes(g.next_frame("I")) for g in gens], cfg, label=f"configs[1] picture {i}",
                             mode=backend.RUN_RECON)
