"""Every kernel form the launcher can choose, against the oracle.

The planner (edge264_amd/csrc/e264_plan.cpp e264_plan, fed by e264_backend.hip launch(), executed by e264_kernels.hip e264_launch_frames) picks
different kernels for the same picture depending on
the size and make-up of the submission, the lanes in use and the device options: two workgroups per picture or one for deblocking and for
an all-I batch's intra pass, the split-off intra pass of a mixed batch's I pictures, the parameter kernel's small form when no picture
predicts from list 1, the parameter kernel on the second queue.  Here every picture is compared with Oracle.decode_frame on the whole
slot, and every submission's e264hip_launch_counts must equal what the rules say it chose (expected_forms below: the rule table, written
out here independently of the planner and computed from the device's CU count and the lanes that have live streams;
tests/test_host_logic.py holds the planner to it on the CPU), so a test that means one form cannot silently run another.  The rule boundaries themselves (128 / 129 pictures, 48 / 49 split-off I pictures, 320 / 321 others on a 256-CU device) are
taken with pictures of a few macroblocks."""
import contextlib
import json
import os
import zipfile
from collections import Counter

import numpy as np
import pytest

from edge264_amd import backend, packet as P, synth
from tests.test_hip_parity import CASES, describe_mismatch

HERE = os.path.dirname(os.path.abspath(__file__))
CORPUS = os.path.join(HERE, "golden", "corpus", "gpu_corpus_sample.zip")
DEFAULTS = dict(split_planes=1, split_intra=1, side_queue=0, waves=108, intra_waves=16)
HOWS = ["resident", "host", "pinned", "pinned_untrusted"]
WIRE_VERSIONS = (P.E264_VERSION_COMPACT, P.E264_VERSION_COMPACT2)  # both levels of the fold go through the expansion kernel


# ---- the launcher's rules, written out -------------------------------------------------------------------------

def packet_info(v4: bytes, sent: bytes, how: str):
    """(prediction work, list-1 motion) of a picture as the submission path sees it: a trusted batch (pinned) does not walk the records of a
    wire packet and counts it as having prediction work"""
    pk = P.Packet(v4)
    kind = pk.mbs["kind"]
    inter = np.nonzero(kind == P.MB_INTER)[0]
    l1 = bool(len(inter) and (pk.motion["refPic"][inter, 4:] >= 0).any())
    pw = bool(len(inter) or (kind == P.MB_PCM).any())
    if how == "pinned" and sent[4] in WIRE_VERSIONS:
        pw = True
    return pw, l1


def expected_forms(infos, cfg, n_cus, max_lane=0, expand=0):
    """Pictures per kernel form for one submission of len(infos) pictures (the rule table of e264_plan, e264_plan.cpp)"""
    c = Counter()
    n = len(infos)
    n_nopred = sum(not pw for pw, _ in infos)
    no_pred = n_nopred == n
    iw = cfg["intra_waves"]
    split = (cfg["split_intra"] == 2 or (cfg["split_intra"] and max_lane < 2)) and 0 < n_nopred < n
    cu_alone = n_cus // (max_lane + 1)
    planes_split = cfg["split_planes"] and split and 2 * n_nopred <= n_cus * 3 // 8 and n - n_nopred <= 320
    planes_alone = cfg["split_planes"] and no_pred and 2 * n <= cu_alone
    planes_dbk = cfg["split_planes"] and 2 * n <= cu_alone
    n_front = n - (n_nopred if split else 0)
    c["expand"] += expand
    if split:
        c["intra_planes_split" if planes_split and iw == 16 else "intra_split"] += n_nopred
    c["dbkp_general" if any(l1 for _, l1 in infos) else "dbkp_small"] += n
    if cfg["side_queue"] and not split:
        c[f"dbkp_side{cfg['side_queue']}"] += n
    if not no_pred:
        c["pred"] += n_front
    if no_pred and planes_alone and iw == 16:
        c["intra_planes_alone"] += n
    else:
        c[f"intra{iw}_{'nobitmap' if no_pred else 'bitmap'}"] += n_front
    w = cfg["waves"]
    if w == 108 and planes_dbk:
        c["dbk_planes"] += n
    else:
        c[f"dbk2_{w - 100}" if w > 100 else f"dbk_{w}"] += n
    return {k: v for k, v in c.items() if v}


def observed(dev, reset=True):
    return {k: v for k, v in dev.launch_counts(reset=reset).items() if v and k != "n_cus"}


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


@contextlib.contextmanager
def options(dev, **kw):
    """device options for a block; every one is restored whatever happens"""
    cfg = dict(DEFAULTS, **kw)
    prev = {}
    try:
        for k, v in kw.items():
            prev[k] = dev.set_option(k, v)
        yield cfg
    finally:
        for k, v in prev.items():
            dev.set_option(k, v)


# ---- one decoder on both sides: the device's slots and the oracle's ------------------------------------------

class Dec:
    def __init__(self, dev, lane=0):
        self.st = backend.Stream(dev, 1, 1)
        if lane:
            self.st.bind_lane(lane)
        self.lane = lane
        self.dpb = [None] * P.MAX_SLOTS

    def prepare(self, v4: bytes):
        """the slots the picture names exist on both sides, filled with 0 (the slot rules of HipFront.decode_capture); a slot too small
        for the picture (the stream's size grew) is allocated again on both sides"""
        h = P.Packet(v4).hdr
        nb = int(h["plane_size_Y"]) + int(h["plane_size_C"])
        for s in range(P.MAX_SLOTS):
            if (s == int(h["dst_slot"]) or int(h["ref_slots"]) >> s & 1) and (self.dpb[s] is None or len(self.dpb[s]) < nb + 64):
                self.st.frame_bytes = nb
                self.st.alloc(s)
                self.st.fill(s, 0)
                self.dpb[s] = np.zeros(nb + 64, np.uint8)

    def check(self, oracle, v4: bytes, label: str):
        pk = P.Packet(v4)
        d, nb = int(pk.hdr["dst_slot"]), pk.frame_bytes()
        oracle.decode_frame(v4, self.dpb, 3)
        self.st.frame_bytes = nb
        got = self.st.download(d)
        assert np.array_equal(got, self.dpb[d][:nb]), f"{label}: " + describe_mismatch(pk, got, self.dpb[d][:nb], pk.width_mbs, pk.height_mbs)

    def close(self):
        self.st.close()


@contextlib.contextmanager
def decoders(dev, n, lanes=(0,)):
    ds = []
    try:
        for k in range(n):
            ds.append(Dec(dev, lanes[k % len(lanes)]))
        yield ds
    finally:
        dev.sync()
        for d in ds:
            d.close()


def submit(dev, how, decs, sent):
    sts = [d.st for d in decs]
    if how == "single":
        for st, p in zip(sts, sent):
            st.submit(p)
    elif how == "resident":
        dps = [dev.upload_packet(p) for p in sent]
        try:
            dev.submit_batch(sts, dps)
        finally:
            for dp in dps:
                dp.free()
    elif how == "host":
        dev.submit_batch_host(sts, sent)
    elif how in ("pinned", "pinned_untrusted"):
        ptrs = [dev.pinned_copy(p) for p in sent]
        try:
            dev.submit_pinned_prepared(dev.prepare_pinned_batch(sts, ptrs, [len(p) for p in sent]), trusted=how == "pinned")
        finally:
            dev.sync()
            for p in ptrs:
                dev.pinned_free(p)
    else:
        raise ValueError(how)


def run_batch(dev, oracle, how, decs, v4s, cfg, sent=None, max_lane=0, label=""):
    """One submission of pictures v4s[k] for decoder decs[k] (sent: the bytes actually submitted, e.g. wire packets), every picture
    compared with the oracle, the forms with the rules.  Returns the forms."""
    sent = sent or v4s
    for d, p in zip(decs, v4s):
        d.prepare(p)
    observed(dev)  # (reset)
    submit(dev, how, decs, sent)
    for k, (d, p) in enumerate(zip(decs, v4s)):
        d.check(oracle, p, f"{label} picture {k} of {len(decs)} ({how})")
    got = observed(dev)
    want = expected_submission(dev, how, v4s, sent, cfg, max_lane)
    assert got == want, f"{label} ({how}): launched {got}, the rules say {want}"
    return got


def expected_submission(dev, how, v4s, sent, cfg, max_lane=0):
    """the forms one submission of v4s (sent: the bytes submitted) must launch, by entry point"""
    cus = dev.launch_counts()["n_cus"]
    wire = [s[4] in WIRE_VERSIONS for s in sent]
    if how == "single":  # (one launch per picture)
        want = Counter()
        for p, s, x in zip(v4s, sent, wire):
            want.update(expected_forms([packet_info(p, s, how)], cfg, cus, max_lane, int(x)))
        return dict(want)
    # (resident packets are unfolded at upload)
    return expected_forms([packet_info(p, s, how) for p, s in zip(v4s, sent)], cfg, cus, max_lane, len(sent) if how != "resident" and any(wire) else 0)


def n_cus(dev):
    return dev.launch_counts()["n_cus"]


# ---- a. the feature matrix on every form ---------------------------------------------------------------------

SETTINGS = {
    "defaults": dict(),
    "split_planes0": dict(split_planes=0),
    "side_queue1": dict(side_queue=1),
    "side_queue2": dict(side_queue=2),
    "waves107": dict(waves=107),
    "waves106": dict(waves=106),
    "waves8": dict(waves=8),
    "waves7": dict(waves=7),
    "waves4": dict(waves=4),
    "waves2": dict(waves=2),
    "intra_waves8": dict(intra_waves=8),
    "intra_waves4": dict(intra_waves=4, split_planes=0),
}
# forms a setting must reach over a case (one of each group)
REACHES = {"defaults": ["dbk_planes"], "split_planes0": ["dbk2_8"], "side_queue1": ["dbkp_side1"], "side_queue2": ["dbkp_side2"],
           "waves107": ["dbk2_7"], "waves106": ["dbk2_6"], "waves8": ["dbk_8"], "waves7": ["dbk_7"], "waves4": ["dbk_4"], "waves2": ["dbk_2"],
           "intra_waves8": ["intra8_bitmap", "intra8_nobitmap", "intra_split"], "intra_waves4": ["intra4_bitmap", "intra4_nobitmap", "intra_split"]}
GEOMS = [(5, 4), (11, 3), (1, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name,pattern,kw", CASES, ids=[c[0] for c in CASES])
def test_feature_matrix_on_every_form(device, oracle, setting, name, pattern, kw):
    """the parity cases of test_hip_parity.py, three streams of different seeds and geometries per submission, under every setting"""
    gens = [synth.StreamSynth(w, h, 700 + 13 * k, **kw) for k, (w, h) in enumerate(GEOMS)]
    total = Counter()
    with options(device, **SETTINGS[setting]) as cfg, decoders(device, len(gens)) as decs:
        for i, t in enumerate(pattern):
            pkts = [bytes(g.next_frame(t)) for g in gens]
            total.update(run_batch(device, oracle, "resident", decs, pkts, cfg, label=f"{name} {setting} frame {i}{t}"))
    assert sum(total[f] for f in REACHES[setting]) > 0, total
    if setting == "split_planes0" and "I" in pattern and not kw.get("pcm_prob"):
        assert total["intra16_nobitmap"] > 0, total


# ---- b. the rule boundaries, with pictures of a few macroblocks ----------------------------------------------

TINY = [(1, 1), (2, 1), (1, 2), (3, 2), (2, 2), (3, 1)]


def tiny_gens(n, seed, pcm=False):
    return [synth.StreamSynth(*TINY[k % len(TINY)], seed=seed + k, intra_in_inter=0.0, pcm_prob=1.0 if pcm else 0.0) for k in range(n)]


def batch(dev, oracle, how, cfg, sel, label, max_lane=0):
    """sel: [(decoder, generator, picture type)] in one submission"""
    pkts = [bytes(g.next_frame(t)) for _, g, t in sel]
    return run_batch(dev, oracle, how, [d for d, _, _ in sel], pkts, cfg, max_lane=max_lane, label=label)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["resident", "host"])
def test_rule_boundaries_on_one_lane(device, oracle, how):
    cus = n_cus(device)
    half = cus // 2  # the largest batch that gets two workgroups per picture: 2 n <= n_cus
    nn = cus * 3 // 16  # the most split-off I pictures that get two workgroups each: 2 n_nopred <= n_cus * 3 / 8
    n_plain = max(2 * half + 1, 322, nn + 101)
    plain, pcm = tiny_gens(n_plain, 1000), tiny_gens(10, 5000, pcm=True)
    with options(device) as cfg, decoders(device, n_plain + 10) as decs:
        dp, dq = decs[:n_plain], decs[n_plain:]
        I = lambda ks, t="I": [(dp[k], plain[k], t) for k in ks]  # noqa: E731
        f = batch(device, oracle, how, cfg, I(range(half)), f"all-I n={half}")
        assert f["intra_planes_alone"] == half and f["dbk_planes"] == half, f
        f = batch(device, oracle, how, cfg, I(range(half, 2 * half + 1)), f"all-I n={half + 1}")
        assert f["intra16_nobitmap"] == half + 1 and f["dbk2_8"] == half + 1 and "intra_planes_alone" not in f, f
        # the rest of the streams' first pictures, with I_PCM pictures among them: those have prediction work and stay in front
        rest = I(range(2 * half + 1, n_plain)) + [(dq[k], pcm[k], "I") for k in range(10)]
        f = batch(device, oracle, how, cfg, rest, "I pictures, ten with I_PCM")
        assert f["pred"] == 10 and f.get("intra_split", 0) + f.get("intra_planes_split", 0) == len(rest) - 10, f
        f = batch(device, oracle, how, cfg, I(range(half), "P"), f"P n={half}")
        assert f["dbk_planes"] == half and f["pred"] == half and f["dbkp_small"] == half, f
        f = batch(device, oracle, how, cfg, I(range(half + 1), "P"), f"P n={half + 1}")
        assert f["dbk2_8"] == half + 1 and "dbk_planes" not in f, f
        # mixed batches: n_nopred at the split-planes budget and one over; the others at 320 and 321; one I picture; one P picture
        f = batch(device, oracle, how, cfg, I(range(nn)) + I(range(nn, nn + 100), "P"), f"mixed {nn} I + 100 P")
        assert f["intra_planes_split"] == nn, f
        f = batch(device, oracle, how, cfg, I(range(nn + 1)) + I(range(nn + 1, nn + 101), "P"), f"mixed {nn + 1} I + 100 P")
        assert f["intra_split"] == nn + 1 and "intra_planes_split" not in f, f
        f = batch(device, oracle, how, cfg, I(range(1)) + I(range(1, 321), "P"), "mixed 1 I + 320 P")
        assert f["intra_planes_split"] == 1, f
        f = batch(device, oracle, how, cfg, I(range(1)) + I(range(1, 322), "P"), "mixed 1 I + 321 P")
        assert f["intra_split"] == 1 and "intra_planes_split" not in f, f
        f = batch(device, oracle, how, cfg, I(range(40)) + I(range(40, 41), "P"), "mixed 40 I + 1 P")
        assert f["intra_planes_split"] == 40 and f["pred"] == 1, f
        f = batch(device, oracle, how, cfg, I(range(30)) + [(dq[k], pcm[k], "I") for k in range(3)], "30 I + 3 I_PCM pictures")
        assert f["intra_planes_split"] == 30 and f["pred"] == 3, f


@pytest.mark.gpu
def test_rule_boundaries_on_two_lanes(device, oracle):
    """streams on lanes 0 and 1: each lane's share of the CUs halves the two-workgroup boundary"""
    cus = n_cus(device)
    q = cus // 2 // 2
    nn = cus * 3 // 16
    per_lane = max(q + 1, nn + 11)
    gens = tiny_gens(2 * per_lane, 2000)
    with options(device) as cfg, decoders(device, 2 * per_lane, lanes=(0, 1)) as decs:
        on = {lane: [(decs[k], gens[k]) for k in range(2 * per_lane) if decs[k].lane == lane] for lane in (0, 1)}
        sel = lambda lane, a, b, t: [(d, g, t) for d, g in on[lane][a:b]]  # noqa: E731
        for lane in (0, 1):
            f = batch(device, oracle, "resident", cfg, sel(lane, 0, q, "I"), f"lane {lane} all-I n={q}", max_lane=1)
            assert f["intra_planes_alone"] == q and f["dbk_planes"] == q, f
            f = batch(device, oracle, "host", cfg, sel(lane, q, per_lane, "I") + sel(lane, 0, 1, "P"), f"lane {lane} mixed", max_lane=1)
            f = batch(device, oracle, "resident", cfg, sel(lane, 0, q + 1, "P"), f"lane {lane} P n={q + 1}", max_lane=1)
            assert f["dbk2_8"] == q + 1, f
            f = batch(device, oracle, "host", cfg, sel(lane, 0, q, "P"), f"lane {lane} P n={q}", max_lane=1)
            assert f["dbk_planes"] == q, f
        f = batch(device, oracle, "resident", cfg, sel(1, 0, nn, "I") + sel(1, nn, nn + 10, "P"), f"lane 1 mixed {nn} I", max_lane=1)
        assert f["intra_planes_split"] == nn, f
        f = batch(device, oracle, "host", cfg, sel(1, 0, nn + 1, "I") + sel(1, nn + 1, nn + 11, "P"), f"lane 1 mixed {nn + 1} I", max_lane=1)
        assert f["intra_split"] == nn + 1, f


# ---- c. what one submission may hold ---------------------------------------------------------------------

COMPOSITION = [((1, 1), "IPBPI"), ((1, 68), "IPPBB"), ((120, 68), "IIPBP"), ((26, 7), "IPIBP"),
               ((26, 7), "IPBPI"), ((1, 1), "IIPBP"), ((120, 68), "IPIBP"), ((1, 68), "IPPBB")]


@pytest.mark.gpu
@pytest.mark.parametrize("how", HOWS)
def test_batch_composition(device, oracle, how):
    """1x1, 1x68, 120x68 and 26x7 pictures, I, P and B, version-4 and wire packets in one submission: grids sized by the largest picture
    with early-exit workgroups, the general parameter kernel, the expansion kernel over version-4 jobs"""
    gens = [synth.StreamSynth(w, h, seed=900 + k, num_refs=2, t8x8=bool(k & 1), intra_in_inter=0.1, p_skip=0.6) for k, ((w, h), _) in enumerate(COMPOSITION)]
    total = Counter()
    with options(device) as cfg, decoders(device, len(gens)) as decs:
        for i in range(len(COMPOSITION[0][1])):
            pkts = [bytes(g.next_frame(gop[i])) for g, (_, gop) in zip(gens, COMPOSITION)]
            sent = [backend.packet_compact(p) if (k + i) & 1 else p for k, p in enumerate(pkts)]
            total.update(run_batch(device, oracle, how, decs, pkts, cfg, sent=sent, label=f"composition {i}"))
    assert total["dbkp_general"] > 0 and total["pred"] > 0, total
    if how != "resident":
        assert total["expand"] == len(gens) * len(COMPOSITION[0][1]), total


# ---- d. list-1 detection ---------------------------------------------------------------------------------

def rebuild(raw: bytes, edit) -> bytes:
    """A version-4 packet rebuilt from its parsed parts after edit(builder); header summaries follow the records"""
    pk = P.Packet(raw)
    h = pk.hdr
    b = P.PacketBuilder(pk.width_mbs, pk.height_mbs, int(h["dst_slot"]), int(h["frame_id"]))
    b.slices = [s for s in np.array(pk.slices)]
    b.mbs = pk.mbs.copy()
    b.motion = pk.motion.copy() if pk.motion is not None else b.motion
    b.payload = bytearray(pk.data[pk.payload_off:pk.payload_off + int(h["payload_bytes"])])
    edit(b)
    inter = np.nonzero(b.mbs["kind"] == P.MB_INTER)[0]
    b.ref_slots = 0
    for r in np.unique(b.motion["refPic"][inter]) if len(inter) else []:
        if r >= 0:
            b.ref_slots |= 1 << int(r)
    return b.finish()


def _l0_only(b, keep_last):
    """every inter macroblock but the last on list 0 alone (a list-1-only one takes its list-1 motion as list 0)"""
    mo = b.motion
    for a in np.nonzero(b.mbs["kind"] == P.MB_INTER)[0]:
        if keep_last and a == len(b.mbs) - 1:
            continue
        m = mo[a]
        mv = m["mvs"].reshape(2, 16, 2)
        for q in range(4):
            if m["refPic"][q] < 0 and m["refPic"][4 + q] >= 0:
                m["refPic"][q], m["refIdx"][q] = m["refPic"][4 + q], 0
                mv[0, 4 * q:4 * q + 4] = mv[1, 4 * q:4 * q + 4]
        m["refPic"][4:], m["refIdx"][4:] = -1, -1
        mv[1] = 0


def _plain_last(b, l0, l1, l1_quadrants, mvs1):
    """the last macroblock: no residual, list-0 motion `l0` (slot or None) over all four quadrants, list-1 motion from slot l1 over
    `l1_quadrants` with the vectors mvs1 (16 x 2) -- and its left and upper neighbours inter, without residual, with the same list-0 motion"""
    w = b.w
    last = len(b.mbs) - 1
    for a in (last, last - 1, last - w):
        if a < 0:
            continue
        m = b.mbs[a]
        m["kind"], m["coded"], m["nz_mask"] = P.MB_INTER, 0, 0
        m["flags"] &= P.MBF_EDGE_LEFT | P.MBF_EDGE_TOP | P.MBF_DEBLOCK
        mo = b.motion[a]
        mo["refPic"], mo["refIdx"], mo["mvs"] = -1, -1, 0
        if l0 is not None or a != last:
            mo["refPic"][:4], mo["refIdx"][:4] = l0 if l0 is not None else l1, 0
            mo["mvs"].reshape(2, 16, 2)[0] = (4, -8)
    mo = b.motion[last]
    for q in l1_quadrants:
        mo["refPic"][4 + q], mo["refIdx"][4 + q] = l1, 0
    mo["mvs"].reshape(2, 16, 2)[1] = mvs1


def list1_variants(seed=41):
    """(name, version-4 B picture whose only list-1 use is its last macroblock, the same with that list-1 motion dropped or None,
    wire form or None) + the packets before it (I, P) + a P picture of the same stream for P-only batches"""
    g = synth.StreamSynth(6, 4, seed, intra_in_inter=0.0, p_skip=0.9, residual_prob=0.2, num_refs=2)
    before = [bytes(g.next_frame(t)) for t in "IP"]
    b_pic = bytes(g.next_frame("B"))
    r0 = int(P.Packet(before[0]).hdr["dst_slot"])
    r1 = int(P.Packet(before[1]).hdr["dst_slot"])
    uni = np.tile(np.array([12, 20], np.int16), (16, 1))
    quad = np.array([[12 + 4 * (j & 1), 20 - 4 * (j >> 1)] for j in range(16)], np.int16)  # four vectors in quadrant 3: sub-8x8

    def make(l0, quadrants, mvs1, drop=False):
        def edit(b):
            _l0_only(b, keep_last=True)
            _plain_last(b, l0, r1, [] if drop else quadrants, mvs1)
        return rebuild(b_pic, edit)

    out = []
    # 1: list 0 and list 1 over the whole macroblock (the uniform list-1 bit); dropped: list 0 alone
    out.append(("uniform", make(r0, range(4), uni), make(r0, range(4), uni, drop=True), None))
    # 2: list 1 in quadrant 3 only, four vectors there (a quadrant bit); dropped: list 0 alone
    v2 = make(r0, [3], quad)
    out.append(("quadrant", v2, make(r0, [3], quad, drop=True), None))
    # 3: list 1 alone, 16x16, no residual: a compact entry with E264_MBCF_LIST1 in the wire form
    v3 = make(None, range(4), uni)
    out.append(("compact_list1", v3, None, backend.packet_compact(v3)))
    # 4: variant 2 in the wire form: a full record behind the compact entries of the skipped macroblocks
    out.append(("wire_full_record", v2, None, backend.packet_compact(v2)))
    p_pic = bytes(g.next_frame("P"))
    return before, out, p_pic


def _wire_layout(wire: bytes):
    """(is the last macroblock a compact entry, the flags byte of its entry, compact entries before it)"""
    h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
    wm, hm, mo = int(h["width_mbs"]), int(h["height_mbs"]), int(h["mbs_off"])
    wpr = int.from_bytes(wire[mo + 12:mo + 16], "little")
    cbits = np.frombuffer(wire, "<u4", hm * wpr, mo + 16 + 12 * hm)
    last = (hm - 1) * wpr + ((wm - 1) >> 5)
    n_compact = int.from_bytes(wire[mo:mo + 4], "little")
    return bool(cbits[last] >> ((wm - 1) & 31) & 1), n_compact


def test_list1_variants_are_what_they_claim(oracle):
    """(CPU) each variant holds list-1 motion in its last macroblock only, in the record form it names, and list-1 motion there decides bS
    (the oracle's bS with that motion dropped differs): a parameter kernel that ignored it would deblock differently"""
    before, variants, p_pic = list1_variants()
    for name, v4, dropped, wire in variants:
        assert backend.packet_check(v4) == 0, name
        pk = P.Packet(v4)
        inter = np.nonzero(pk.mbs["kind"] == P.MB_INTER)[0]
        with_l1 = [int(a) for a in inter if (pk.motion["refPic"][a, 4:] >= 0).any()]
        assert with_l1 == [len(pk.mbs) - 1], (name, with_l1)
        h = int(np.ascontiguousarray(pk.mbs["modes"][-1]).view("<u4")[1])
        if name == "uniform":
            assert h >> 9 & 1 and h >> 4 & 15 == 15
        if name in ("quadrant", "wire_full_record"):
            assert not h >> 9 & 1 and h >> 4 & 15 == 8
        if dropped is not None:
            n = len(pk.mbs)
            assert not np.array_equal(oracle.frame_bs(v4, n), oracle.frame_bs(dropped, n)), name
        if wire is not None:
            assert wire[4] == P.E264_VERSION_COMPACT and backend.packet_check(wire) == 0
            last_compact, n_compact = _wire_layout(wire)
            assert n_compact >= 3, name
            assert last_compact == (name == "compact_list1"), name
            mo = int(np.frombuffer(wire, P.FRAME_HDR, 1)[0]["mbs_off"])
            assert int.from_bytes(wire[mo + 4:mo + 8], "little") == 0, name  # no two-list entry: the trusted scan walks the entries
    assert not (P.Packet(p_pic).motion["refPic"][:, 4:] >= 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("how", HOWS)
def test_list1_detection(device, oracle, how):
    """a B picture whose only list-1 use is one macroblock, last in raster order, takes the general parameter kernel; a P-only batch the
    small one"""
    before, variants, _ = list1_variants()
    helpers = [synth.StreamSynth(4, 3, seed=60 + k, intra_in_inter=0.0) for k in range(2)]
    with options(device) as cfg, decoders(device, len(variants) + 2) as decs:
        run_batch(device, oracle, how, decs[:len(variants)] + decs[-2:], [before[0]] * len(variants) + [bytes(h.next_frame("I")) for h in helpers], cfg, label="I")
        run_batch(device, oracle, how, decs[:len(variants)], [before[1]] * len(variants), cfg, label="P")
        for k, (name, v4, _, wire) in enumerate(variants):
            sent = [wire or v4] + [bytes(h.next_frame("P")) for h in helpers]
            v4s = [v4] + sent[1:]
            f = run_batch(device, oracle, how, [decs[k]] + decs[-2:], v4s, cfg, sent=sent, label=name)
            assert f["dbkp_general"] == 3 and "dbkp_small" not in f, (name, f)
        f = run_batch(device, oracle, how, decs[-2:], [bytes(h.next_frame("P")) for h in helpers], cfg, label="P only")
        assert f["dbkp_small"] == 2 and "dbkp_general" not in f, f


# ---- e. the corpus sample in large batches ----------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus_captures():
    """the packets of every stream of the sample, captured on the host, in version-4 and wire form"""
    from edge264_amd import front
    z = zipfile.ZipFile(CORPUS)
    index = json.loads(z.read("index.json"))
    out = []
    for c in index:
        data = z.read(c["file"])
        v4, _, _ = front.capture_packets(data)
        wire, _, _ = front.capture_packets(data, compact=True)
        assert len(v4) == len(wire), c["file"]
        if v4:
            out.append((c["file"], v4, wire))
    front.load().e264front_set_compact(0)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["version4", "wire"])
def test_corpus_in_large_batches(device, oracle, corpus_captures, form):
    """the k-th packet of every stream of the sample in one submission: up to 500 pictures of mixed geometry, CAVLC / CABAC, MVC and
    damaged streams (the first packets in two: those without prediction work, then the others); with the defaults, then with one
    workgroup per picture and no split"""
    caps = corpus_captures
    total = Counter()
    how = "resident" if form == "version4" else "host"
    for opts in (dict(), dict(split_planes=0, split_intra=0)):
        with options(device, **opts) as cfg, decoders(device, len(caps)) as decs:
            for k in range(max(len(c[1]) for c in caps)):
                ks = [i for i, c in enumerate(caps) if k < len(c[1])]
                # the first pictures without prediction work (I pictures without I_PCM) go first, in a submission of their own: the all-I batch
                groups = [ks] if k else [[i for i in ks if not packet_info(caps[i][1][0], b"", how)[0]], [i for i in ks if packet_info(caps[i][1][0], b"", how)[0]]]
                for g in (g for g in groups if g):
                    v4s = [caps[i][1][k] for i in g]
                    sent = [caps[i][2][k] for i in g] if form == "wire" else v4s
                    total.update(run_batch(device, oracle, how, [decs[i] for i in g], v4s, cfg, sent=sent, label=f"{form} {opts} packet {k}"))
    for f in ("dbk2_8", "dbk_planes", "intra16_nobitmap"):
        assert total[f] > 0, (f, total)
    assert total["intra_split"] + total["intra_planes_split"] > 0, total
    print(f"corpus in batches ({form}): {sum(len(c[1]) for c in caps)} pictures twice, forms {dict(total)}")


# ---- f. the lanes in use, not the lanes ever used --------------------------------------------------------

@pytest.mark.gpu
def test_lanes_in_use_not_lanes_ever_used(device, oracle):
    cus = n_cus(device)
    with options(device) as cfg:
        g = synth.StreamSynth(3, 2, seed=77)
        with decoders(device, 1, lanes=(3,)) as (d,):
            run_batch(device, oracle, "single", [d], [bytes(g.next_frame("I"))], cfg, max_lane=3, label="lane 3")
        # lane 3 has no stream any more: a lone lane-0 stream has the device to itself
        g = synth.StreamSynth(3, 2, seed=78)
        with decoders(device, 1) as (d,):
            f = run_batch(device, oracle, "single", [d], [bytes(g.next_frame("I"))], cfg, label="lone I")
            assert f["intra_planes_alone"] == 1 and f["dbk_planes"] == 1, f
            f = run_batch(device, oracle, "single", [d], [bytes(g.next_frame("P"))], cfg, label="lone P")
            assert f["dbk_planes"] == 1, f
        gens = tiny_gens(cus // 2, 3000)
        with decoders(device, len(gens)) as decs:
            f = batch(device, oracle, "resident", cfg, [(d, g, "I") for d, g in zip(decs, gens)], f"all-I n={cus // 2} on lane 0")
            assert f["intra_planes_alone"] == cus // 2 and f["dbk_planes"] == cus // 2, f
            f = batch(device, oracle, "resident", cfg, [(decs[0], gens[0], "I"), (decs[1], gens[1], "P")], "I + P on lane 0")
            assert f["intra_planes_split"] == 1 and f["pred"] == 1, f
