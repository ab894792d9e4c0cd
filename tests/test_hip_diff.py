"""The diff kernel on the MI355X (e264hip_frame_diff / e264hip_diff_batch, include/edge264_hip.h): two pictures compared where they lie in HBM.

Views: whole, two crops (Cb at an odd byte; an odd chroma width) and a 2 x 2 corner of pictures of four sizes, A and B in DIFFERENT padded layouts of
tests/layouts.py and in different streams, against diff.frame_diff of the host copies, and again with other random bytes everywhere outside the samples.
Single changes of +-1 at the ends of planes and around a column group's border.  `first` across workgroups.  0 against 255.  A picture against itself.
Ordering behind a submission and a host batch with no wait between.  Batches of 1 to 257 pairs, a mixed batch.  Every refusal.  The front library on cropped,
MVC and 1080p streams with borrowed frames, and the driver's --diff mode.  Everything is compared for equality.  tests/test_diff.py runs the kernel's body on
the host first."""
import ctypes as C
import errno
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, diff as DF, digest as D, packet as P, synth
from tests import layouts as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STREAMS = os.path.join(HERE, "golden", "streams")
EXE = os.path.join(ROOT, "edge264_amd", "e264_multi")
FRONT = os.path.join(ROOT, "edge264_amd", "libedge264_hipfront.so")
HIP = os.path.join(ROOT, "edge264_amd", "libedge264_hip.so")
FRONT_DIGEST = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
NONE = backend.DIFF_NONE
ZERO = dict(sad=0, sse=0, count=0, first=NONE, max=0)


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def geo_of(w, h, layout):
    return dict(width_mbs=w, height_mbs=h, **L.geometry(w, h, layout))


def views_of(w, h, geo):
    """the four views of tests/test_hip_preview.py: whole; a crop with Cb at an odd byte; a crop to an odd chroma width; the bottom-right 2 x 2 luma /
    1 x 1 chroma corner"""
    return [D.frame_view(w, h, geometry=geo), D.frame_view(w, h, crop=(2, 6, 2, 10), geometry=geo), D.frame_view(w, h, crop=(6, 0, 2, 0), geometry=geo),
            D.frame_view(w, h, crop=(w * 16 - 2, 0, h * 16 - 2, 0), geometry=geo)]


def dicts(rec):
    """a device record of one picture (shape (3,)) as diff.frame_diff gives it; the padding member is zero"""
    assert rec.shape == (3,) and rec.dtype == backend.DIFF_DTYPE and not rec["zero"].any()
    return DF.as_dicts(rec)


class Slot:
    """one stream with slots of one padded layout (guard behind, tests/layouts.py), uploaded in full from host images"""

    def __init__(self, dev, w, h, layout, lane=0, n_slots=1):
        self.geo = geo_of(w, h, layout)
        self.w, self.h = w, h
        self.st = backend.Stream(dev, w, h)
        if lane:
            self.st.bind_lane(lane)
        self.bytes = self.st.frame_bytes = L.slot_bytes(self.geo)
        for s in range(n_slots):
            self.st.alloc(s)

    def upload(self, img, slot=0):
        assert len(img) == self.bytes
        self.st.upload(slot, img)

    def close(self):
        self.st.close()


def plane_index(geo, p, i):
    """the byte of a slot image that holds sample i (row-major over the WHOLE picture) of plane p"""
    W = geo["width_mbs"] * 16 >> (p > 0)
    y, x = divmod(i, W)
    if p == 0:
        return y * geo["stride_Y"] + x
    return geo["plane_size_Y"] + y * geo["stride_C"] + x + (geo["stride_C"] // 2 if p == 2 else 0)


def in_layout(img_a, geo_a, geo_b, rng):
    """the samples of a slot image of layout A in a slot image of layout B, every other byte random"""
    b = L.random_slot(geo_b, rng)
    ya, ca = L.samples(geo_a, img_a)
    L.samples(geo_b, b)[0][:] = ya  # (luma is a view of b's bytes; [Cb | Cr] is a copy: chroma is written row by row below)
    W, H = geo_b["width_mbs"] * 16, geo_b["height_mbs"] * 16
    sc, psy = geo_b["stride_C"], geo_b["plane_size_Y"]
    c = b[psy:psy + sc * (H // 2)].reshape(H // 2, sc)
    c[:, :W // 2] = ca[:, :W // 2]
    c[:, sc // 2:sc // 2 + W // 2] = ca[:, W // 2:]
    return b


PAIRS = [("tight", "gaps_wide"), ("gaps_wide", "tight"), ("pad16", "canvas"), ("canvas", "pad16")]
PICTURES = [(w, h, la, lb) for (w, h) in ((1, 1), (5, 3), (17, 5), (130, 5)) for la, lb in PAIRS] + [(120, 68, "tight", "pad16")]


@pytest.mark.parametrize("w,h,la,lb", PICTURES, ids=[f"{w}x{h}-{la}-{lb}" for w, h, la, lb in PICTURES])
def test_views(device, w, h, la, lb):
    """whole, cropped and corner views of A and B in different layouts and streams: the device's records are frame_diff of the host copies, singly and as a
    batch of four, and depend on the samples only"""
    rng = np.random.default_rng(w * 1000 + h + len(la))
    a, b = Slot(device, w, h, la), Slot(device, w, h, lb)
    try:
        va, vb = views_of(w, h, a.geo), views_of(w, h, b.geo)
        assert va[1]["offset"][1] & 1 and va[2]["width"][1] & 1 and va[3]["width"] == [2, 1, 1]
        assert all(backend.diff_check(x, a.bytes, y, b.bytes) == 0 for x, y in zip(va, vb))
        img_a = L.random_slot(a.geo, rng)
        img_b = in_layout(img_a, a.geo, b.geo, rng)
        # a handful of random changes per plane, some of them inside the corner view
        for p in range(3):
            n = (w * 16 >> (p > 0)) * (h * 16 >> (p > 0))
            for i in list(rng.integers(0, n, 5)) + [n - 1]:
                img_b[plane_index(b.geo, p, int(i))] ^= int(rng.integers(1, 256))
        want = [DF.frame_diff(x, img_a, y, img_b) for x, y in zip(va, vb)]
        assert all(r["count"] >= 1 for r in want[0]) and all(r["count"] == 1 for r in want[3][1:])
        a.upload(img_a)
        b.upload(img_b)
        got = device.diff_batch([a.st] * 4, [0] * 4, va, [b.st] * 4, [0] * 4, vb)
        assert got.shape == (4, 3)
        for i in range(4):
            assert dicts(got[i]) == want[i], i
            assert dicts(a.st.diff(0, va[i], b.st, 0, vb[i])) == want[i], i
        # the other way round: the same but for nothing (|a - b| is symmetric)
        assert dicts(b.st.diff(0, vb[1], a.st, 0, va[1])) == want[1]
        # the same samples, other random bytes in the padding, the gaps and the guard of both
        img_a2, img_b2 = L.random_slot(a.geo, rng, samples_from=img_a), L.random_slot(b.geo, rng, samples_from=img_b)
        assert not np.array_equal(img_a, img_a2) and not np.array_equal(img_b, img_b2)
        a.upload(img_a2)
        b.upload(img_b2)
        got = device.diff_batch([a.st] * 4, [0] * 4, va, [b.st] * 4, [0] * 4, vb)
        for i in range(4):
            assert dicts(got[i]) == want[i], (i, "padding")
    finally:
        a.close()
        b.close()


def test_single_changes(device):
    """17 x 5 macroblocks, pad16 against tight: +-1 at each plane's index 0, its last index and the columns 15 / 16 / w - 1 of a middle row gives exactly
    count 1, sad 1, sse 1, max 1, first i, and the other planes are zero with NONE"""
    rng = np.random.default_rng(175)
    w, h = 17, 5
    a, b = Slot(device, w, h, "pad16"), Slot(device, w, h, "tight")
    try:
        va, vb = D.frame_view(w, h, geometry=a.geo), D.frame_view(w, h, geometry=b.geo)
        img_a = L.random_slot(a.geo, rng)
        m = L.sample_mask(a.geo)
        img_a[m] = np.clip(img_a[m], 1, 254)  # every sample can move by 1 either way
        base_b = in_layout(img_a, a.geo, b.geo, rng)
        a.upload(img_a)
        for p in range(3):
            W, H = w * 16 >> (p > 0), h * 16 >> (p > 0)
            row = (H // 2) * W
            for i in (0, W * H - 1, row + 15, row + 16, row + W - 1):
                for step in (1, -1):
                    img_b = base_b.copy()
                    at = plane_index(b.geo, p, i)
                    img_b[at] = int(img_b[at]) + step
                    b.upload(img_b)
                    got = dicts(a.st.diff(0, va, b.st, 0, vb))
                    want = [dict(ZERO)] * 3
                    want[p] = dict(sad=1, sse=1, count=1, first=i, max=1)
                    assert got == want, (p, i, step)
    finally:
        a.close()
        b.close()


@pytest.fixture(scope="module")
def hd_pair(device):
    """two 1080p-sized slots (120 x 68 macroblocks, tight and pad16) with one random picture in both"""
    rng = np.random.default_rng(1080)
    a, b = Slot(device, 120, 68, "tight"), Slot(device, 120, 68, "pad16")
    img_a = L.random_slot(a.geo, rng)
    img_b = in_layout(img_a, a.geo, b.geo, rng)
    a.upload(img_a)
    yield a, b, img_a, img_b
    a.close()
    b.close()


def test_first_across_workgroups(device, hd_pair):
    """120 x 68: a change in the last row and one in row 3 give `first` as row 3's index, whichever workgroup finishes first; the last-row change alone gives its own"""
    a, b, img_a, base_b = hd_pair
    va, vb = D.frame_view(120, 68, geometry=a.geo), D.frame_view(120, 68, geometry=b.geo)
    for p in range(3):
        W, H = 1920 >> (p > 0), 1088 >> (p > 0)
        late, early = (H - 1) * W + 1001 % W, 3 * W + 77
        img_b = base_b.copy()
        img_b[plane_index(b.geo, p, late)] ^= 0x10
        b.upload(img_b)
        got = dicts(a.st.diff(0, va, b.st, 0, vb))
        assert got[p] == dict(sad=16, sse=256, count=1, first=late, max=16) and all(got[q] == ZERO for q in range(3) if q != p), p
        img_b[plane_index(b.geo, p, early)] ^= 0x01
        b.upload(img_b)
        got = dicts(a.st.diff(0, va, b.st, 0, vb))
        assert got[p] == dict(sad=17, sse=257, count=2, first=early, max=16) and all(got[q] == ZERO for q in range(3) if q != p), p
    b.upload(base_b)
    assert dicts(a.st.diff(0, va, b.st, 0, vb)) == [ZERO] * 3


def test_extremes(device, hd_pair):
    """120 x 68: 0 against 255 everywhere gives sad = 255 n, sse = 65025 n, count = n, max 255, first 0 per plane"""
    a, b, img_a, base_b = hd_pair
    va, vb = D.frame_view(120, 68, geometry=a.geo), D.frame_view(120, 68, geometry=b.geo)
    try:
        a.st.fill(0, 0)
        b.st.fill(0, 255)
        for x, y, xv, yv in ((a, b, va, vb), (b, a, vb, va)):
            got = dicts(x.st.diff(0, xv, y.st, 0, yv))
            for p, n in enumerate((1920 * 1088, 960 * 544, 960 * 544)):
                assert got[p] == dict(sad=255 * n, sse=65025 * n, count=n, first=0, max=255), p
    finally:
        a.upload(img_a)
        b.upload(base_b)


def test_same_picture(device):
    """a picture against itself (same stream, slot and view) is all zero with NONE; two slots of one stream work; the defaults of Stream.diff"""
    rng = np.random.default_rng(55)
    s = Slot(device, 5, 3, "pad16", n_slots=2)
    st = backend.Stream(device, 5, 3)  # the reference's layout: Stream.diff's default views
    try:
        views = views_of(5, 3, s.geo)
        img0, img1 = L.random_slot(s.geo, rng), L.random_slot(s.geo, rng)
        s.upload(img0, 0)
        s.upload(img1, 1)
        for v in views:
            assert dicts(s.st.diff(0, v, s.st, 0, v)) == [ZERO] * 3
            assert dicts(s.st.diff(0, v, s.st, 1, v)) == DF.frame_diff(v, img0, v, img1)
        st.alloc(0)
        st.alloc(1)
        i0, i1 = (rng.integers(0, 256, st.frame_bytes, dtype=np.uint8) for _ in range(2))
        st.upload(0, i0)
        st.upload(1, i1)
        v = D.frame_view(5, 3)
        assert dicts(st.diff(0)) == [ZERO] * 3
        assert dicts(st.diff(0, other_slot=1)) == DF.frame_diff(v, i0, v, i1)
    finally:
        s.close()
        st.close()


def smoke_gop(seed=1):
    return synth.StreamSynth(8, 6, seed, t8x8=True, weighted=1, i_kinds=(P.MB_I8x8, P.MB_I4x4, P.MB_I16x16))


@pytest.fixture(scope="module")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def open_smoke_stream(dev, lane=0):
    w, h = 8, 6
    st = backend.Stream(dev, w, h)
    if lane:
        st.bind_lane(lane)
    nb = P.frame_bytes(w, h)
    dpb = [np.full(nb + 16, 128, np.uint8) for _ in range(6)] + [None] * 26
    for i in range(6):
        st.alloc(i)
        st.upload(i, dpb[i][:nb])
    return st, dpb, nb


def open_plain_stream(dev, lane=0):
    st = backend.Stream(dev, 8, 6)
    if lane:
        st.bind_lane(lane)
    st.alloc(0)
    return st


@pytest.mark.parametrize("lane", [0, 2])
def test_ordering_behind_a_submission(device, oracle, lane):
    """the oracle's picture uploaded into stream B, the packet submitted to stream A, the diff asked for with nothing between: all zero, for I, P and B;
    then one byte of B flipped: count 1"""
    st, dpb, nb = open_smoke_stream(device, lane)
    other = open_plain_stream(device, lane)
    try:
        view = D.frame_view(8, 6)
        gen = smoke_gop()
        for t in "IPB":
            pkt = gen.next_frame(t)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            oracle.decode_frame(pkt, dpb, 3)
            other.upload(0, dpb[d][:nb])
            st.submit(pkt)
            assert dicts(st.diff(d, view, other, 0, view)) == [ZERO] * 3, t
            flipped = dpb[d][:nb].copy()
            at = view["offset"][1] + 5 * view["stride"][1] + 7
            flipped[at] ^= 0x80
            other.upload(0, flipped)
            assert dicts(st.diff(d, view, other, 0, view)) == [ZERO, dict(sad=128, sse=128 * 128, count=1, first=5 * 64 + 7, max=128), ZERO], t
    finally:
        st.close()
        other.close()


def test_ordering_behind_a_host_batch(device, oracle):
    """submit_batch_host of three streams, then diff_batch of the three against the oracle's pictures in three other streams, with nothing between"""
    sts = [open_smoke_stream(device) for _ in range(3)]
    others = [open_plain_stream(device) for _ in range(3)]
    try:
        gens = [smoke_gop(seed) for seed in (1, 2, 3)]
        view = D.frame_view(8, 6)
        for t in "IPB":
            pkts = [g.next_frame(t) for g in gens]
            dst = [int(P.Packet(p).hdr["dst_slot"]) for p in pkts]
            for j, (st, dpb, nb) in enumerate(sts):
                oracle.decode_frame(pkts[j], dpb, 3)
                img = dpb[dst[j]][:nb].copy()
                if j == 1:
                    img[view["offset"][0] + 11] ^= 1  # the second pair differs in one luma sample
                others[j].upload(0, img)
            device.submit_batch_host([s[0] for s in sts], pkts)
            got = device.diff_batch([s[0] for s in sts], dst, [view] * 3, others, [0] * 3, [view] * 3)
            assert dicts(got[0]) == [ZERO] * 3 and dicts(got[2]) == [ZERO] * 3, t
            assert dicts(got[1]) == [dict(sad=1, sse=1, count=1, first=11, max=1), ZERO, ZERO], t
    finally:
        for s in sts:
            s[0].close()
        for s in others:
            s.close()


@pytest.fixture(scope="module")
def tiny_streams(device):
    """257 streams of 1 x 1-macroblock pictures with two slots each, distinct contents, and what the record of slot 0 against slot 1 must be; every fourth pair is equal"""
    rng = np.random.default_rng(257)
    geo = geo_of(1, 1, "tight")
    view = D.frame_view(1, 1, geometry=geo)
    slots, want = [], []
    for k in range(257):
        s = Slot(device, 1, 1, "tight", n_slots=2)
        img0 = L.random_slot(geo, rng)
        img1 = img0.copy() if k % 4 == 0 else L.random_slot(geo, rng, samples_from=img0)
        for _ in range(k % 4):
            img1[int(rng.integers(0, 384))] ^= int(rng.integers(1, 256))
        s.upload(img0, 0)
        s.upload(img1, 1)
        slots.append(s)
        want.append(DF.frame_diff(view, img0, view, img1))
    assert want[0] == [ZERO] * 3 and len({json.dumps(w) for w in want}) > 150
    yield slots, view, want
    for s in slots:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_batches_of_small_pictures(device, tiny_streams, n):
    slots, view, want = tiny_streams
    sts = [s.st for s in slots[:n]]
    got = device.diff_batch(sts, [0] * n, [view] * n, sts, [1] * n, [view] * n)
    assert got.shape == (n, 3) and all(dicts(got[i]) == want[i] for i in range(n))
    # results come in call order: the same pairs the other way round
    got = device.diff_batch(sts[::-1], [0] * n, [view] * n, sts[::-1], [1] * n, [view] * n)
    assert all(dicts(got[i]) == want[n - 1 - i] for i in range(n))


def test_mixed_batch(device):
    """pairs of four sizes in one call, each stream in its own layout, a stream appearing on both sides, equal and unequal pairs interleaved, whole and cropped views"""
    rng = np.random.default_rng(77)
    sizes = [(1, 1), (5, 3), (17, 5), (130, 5)]
    slots = [Slot(device, *sizes[i % 4], L.MIXED[i % len(L.MIXED)]) for i in range(8)]  # streams i and i + 4 hold pictures of one size in two layouts
    try:
        imgs = []
        for i, s in enumerate(slots):
            if i < 4:
                img = L.random_slot(s.geo, rng)
            else:
                img = in_layout(imgs[i - 4], slots[i - 4].geo, s.geo, rng)
                if i & 1:  # (pairs 1 and 3 differ, 0 and 2 are equal)
                    for p in range(3):
                        img[plane_index(s.geo, p, int(rng.integers(0, 64)))] ^= int(rng.integers(1, 256))
            s.upload(img)
            imgs.append(img)
        sa, sb, va, vb, ia, ib = [], [], [], [], [], []
        for i in range(4):
            x, y = slots[i], slots[i + 4]
            for k in range(3):
                sa.append(x); sb.append(y); va.append(views_of(x.w, x.h, x.geo)[k]); vb.append(views_of(y.w, y.h, y.geo)[k]); ia.append(i); ib.append(i + 4)
            # the other way round, and the stream against itself: slots[i] on both sides of one call
            sa.append(y); sb.append(x); va.append(views_of(y.w, y.h, y.geo)[0]); vb.append(views_of(x.w, x.h, x.geo)[0]); ia.append(i + 4); ib.append(i)
            sa.append(x); sb.append(x); va.append(views_of(x.w, x.h, x.geo)[1]); vb.append(views_of(x.w, x.h, x.geo)[1]); ia.append(i); ib.append(i)
        got = device.diff_batch([s.st for s in sa], [0] * len(sa), va, [s.st for s in sb], [0] * len(sb), vb)
        assert got.shape == (20, 3)
        want = [DF.frame_diff(va[k], imgs[ia[k]], vb[k], imgs[ib[k]]) for k in range(20)]
        for k in range(20):
            assert dicts(got[k]) == want[k], k
        assert want[0] == [ZERO] * 3 and all(r["count"] for r in want[5]) and want[4] == [ZERO] * 3
    finally:
        for s in slots:
            s.close()


def test_errors(device):
    """every refusal is EINVAL with a text, leaves `out` untouched and queues nothing: a valid call right after it gives the right record"""
    lib = device.L
    rng = np.random.default_rng(9)
    a, b, other_lane, small = Slot(device, 5, 3, "pad16"), Slot(device, 5, 3, "tight"), Slot(device, 5, 3, "pad16", lane=1), Slot(device, 1, 1, "tight")
    dev2 = backend.Device(0)  # a second device object: its streams are not `device`'s
    foreign = Slot(dev2, 5, 3, "tight")
    try:
        img_a = L.random_slot(a.geo, rng)
        img_b = L.random_slot(b.geo, rng)
        a.upload(img_a)
        b.upload(img_b)
        other_lane.upload(img_a)
        foreign.upload(img_b)
        small.upload(L.random_slot(small.geo, rng))
        va, vb = views_of(5, 3, a.geo)[1], views_of(5, 3, b.geo)[1]
        want = DF.frame_diff(va, img_a, vb, img_b)
        ca, cb = backend.as_view(va), backend.as_view(vb)
        out = np.full((2, 3), 7, backend.DIFF_DTYPE)
        untouched = out.copy()

        def call(dev=device.h, streams_a=(a.st.h,), slots_a=(0,), views_a=(ca,), streams_b=(b.st.h,), slots_b=(0,), views_b=(cb,), n=None, res=out.ctypes.data):
            m = len(streams_a) if streams_a is not None else 1
            arr = lambda t, x: (t * len(x))(*x) if x is not None else None
            return lib.e264hip_diff_batch(dev, arr(C.c_void_p, streams_a), arr(C.c_int, slots_a), arr(backend.View, views_a),
                                          arr(C.c_void_p, streams_b), arr(C.c_int, slots_b), arr(backend.View, views_b), m if n is None else n, res)

        def refused(what, **kw):
            assert call(**kw) == errno.EINVAL, what
            assert backend.last_error(), what
            assert (out == untouched).all(), what
            assert dicts(a.st.diff(0, va, b.st, 0, vb)) == want, f"after the refusal of {what}"

        refused("a null device", dev=None)
        for name in ("streams_a", "slots_a", "views_a", "streams_b", "slots_b", "views_b"):
            refused("null " + name, **{name: None})
        refused("null out", res=None)
        refused("a null stream of A", streams_a=(None,))
        refused("a null stream of B", streams_b=(None,))
        refused("n < 0", n=-1)
        refused("n > 4096", n=4097)
        for side in ("slots_a", "slots_b"):
            refused(side + ": slot -1", **{side: (-1,)})
            refused(side + ": slot past the table", **{side: (P.MAX_SLOTS,)})
            refused(side + ": a slot that is not allocated", **{side: (5,)})
        refused("streams of two lanes across the two sides", streams_b=(other_lane.st.h,), views_b=(ca,))
        refused("streams of two lanes on side A", streams_a=(a.st.h, other_lane.st.h), slots_a=(0, 0), views_a=(ca, ca), streams_b=(b.st.h, b.st.h), slots_b=(0, 0), views_b=(cb, cb))
        refused("streams of two lanes on side B", streams_a=(a.st.h, a.st.h), slots_a=(0, 0), views_a=(ca, ca), streams_b=(b.st.h, other_lane.st.h), slots_b=(0, 0), views_b=(cb, ca))
        refused("a stream of another device on side B", streams_b=(foreign.st.h,))
        refused("a stream of another device on side A", streams_a=(foreign.st.h,), views_a=(cb,))
        for side, good in (("views_a", ca), ("views_b", cb)):
            bad = backend.as_view(good)
            bad.plane[2].height += 4096
            refused(side + ": a view that leaves the slot", **{side: (bad,)})
            bad = backend.as_view(good)
            bad.plane[1].width = 0
            refused(side + ": a plane without samples", **{side: (bad,)})
            bad = backend.as_view(good)
            bad.plane[0].stride = bad.plane[0].width - 1
            refused(side + ": a stride below the width", **{side: (bad,)})
        bad = backend.as_view(cb)
        bad.plane[1].width = 0
        refused("the second pair's view", streams_a=(a.st.h, a.st.h), slots_a=(0, 0), views_a=(ca, ca), streams_b=(b.st.h, b.st.h), slots_b=(0, 0), views_b=(cb, bad))
        # plane sizes that differ in luma only and in chroma only
        luma = backend.as_view(cb)
        luma.plane[0].width -= 2
        refused("luma widths differ", views_b=(luma,))
        luma = backend.as_view(cb)
        luma.plane[0].height -= 2
        refused("luma heights differ", views_b=(luma,))
        chroma = backend.as_view(ca)
        chroma.plane[1].height -= 1
        chroma.plane[2].height -= 1
        refused("chroma heights differ", views_a=(chroma,))
        chroma = backend.as_view(cb)
        chroma.plane[2].width -= 1
        refused("Cr widths differ", views_b=(chroma,))
        # a view valid for A's slot but not for B's smaller slot (a picture of one macroblock)
        whole_a = backend.as_view(D.frame_view(5, 3, geometry=b.geo))
        assert backend.view_check(whole_a, b.bytes) == 0 and backend.view_check(whole_a, small.bytes) == errno.EINVAL
        refused("a view valid for A's slot, not for B's smaller one", streams_a=(b.st.h,), views_a=(whole_a,), streams_b=(small.st.h,), views_b=(whole_a,))
        # frame_diff, the batch of one
        o = out.ctypes.data
        assert lib.e264hip_frame_diff(None, 0, C.byref(ca), b.st.h, 0, C.byref(cb), o) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_diff(a.st.h, 0, C.byref(ca), None, 0, C.byref(cb), o) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_diff(a.st.h, 0, None, b.st.h, 0, C.byref(cb), o) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_diff(a.st.h, 0, C.byref(ca), b.st.h, 0, None, o) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_diff(a.st.h, 0, C.byref(ca), b.st.h, 0, C.byref(cb), None) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_diff(a.st.h, 7, C.byref(ca), b.st.h, 0, C.byref(cb), o) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_diff(a.st.h, 0, C.byref(ca), other_lane.st.h, 0, C.byref(ca), o) == errno.EINVAL and backend.last_error()
        with pytest.raises(backend.BackendError):
            a.st.diff(0, va, b.st, 0, luma)
        with pytest.raises(ValueError):
            device.diff_batch([a.st], [0], [va], [b.st], [0], [])
        # n == 0 is no error, with or without arrays
        assert call(n=0) == 0 and call(streams_a=None, slots_a=None, views_a=None, streams_b=None, slots_b=None, views_b=None, n=0, res=None) == 0
        assert device.diff_batch([], [], [], [], [], []).shape == (0, 3)
        assert (out == untouched).all()  # no call above wrote anything
        assert dicts(other_lane.st.diff(0, va, other_lane.st, 0, va)) == [ZERO] * 3  # (the stream of the other lane)
        assert dicts(foreign.st.diff(0, vb, foreign.st, 0, vb)) == [ZERO] * 3        # (... and of the other device object)
    finally:
        for s in (a, b, other_lane, small, foreign):
            s.close()
        dev2.close()


def md5s(frames):
    return [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames]


@pytest.mark.parametrize("download", [1, 0], ids=["download", "no-download"])
@pytest.mark.parametrize("name", ["crop_longterm_mmco", "mvc_ipp", "hd1080_ippb"])
def test_front_end(name, download):
    """e264front_frame_diff over consecutive output frames fetched with borrow = 1 (the earlier one kept until the comparison, then returned), with read-back on
    and off, equals diff_plane over the planes a second, downloading decoder delivered, which are the reference's"""
    from oracle.pyoracle import Edge264Frame, HipFront
    assert os.path.exists(FRONT), f"{FRONT} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    data = open(os.path.join(STREAMS, name + ".264"), "rb").read()
    front = HipFront()
    lib = front.lib
    lib.e264front_set_sink(0)
    frames, _ = front.decode(data)
    assert md5s(frames) == sums[name]["md5"]  # the expectation is the reference's, not the code under test's
    n_views = sums[name]["views"]
    want = [[[DF.diff_plane(p, q) for p, q in zip(cur[3 * v:3 * v + 3], prev[3 * v:3 * v + 3])] for v in range(n_views)] for prev, cur in zip(frames, frames[1:])]
    assert any(r["count"] for fr in want for v in fr for r in v)
    assert os.path.exists(FRONT_DIGEST), f"{FRONT_DIGEST} missing (built by __graft_entry__.build() on every machine)"
    dlib = C.CDLL(FRONT_DIGEST)  # e264front_frame_diff: edge264_amd/frontend/front_diff.c, in the library beside the front library
    dlib.e264front_frame_diff.restype = C.c_int
    dlib.e264front_frame_diff.argtypes = [C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_void_p]
    buf = np.frombuffer(data + b"\0" * 64, np.uint8).copy()
    base, end = buf.ctypes.data, buf.ctypes.data + len(data)
    got, kept = [], []
    lib.e264front_set_download(download)
    try:
        dec = C.c_void_p(lib.edge264_alloc(0, None, None, 0, None, None, None))
        assert dec
        out = Edge264Frame()

        def drain():
            n = 0
            while lib.edge264_get_frame(dec, C.byref(out), 1) == 0:  # borrowed: the frame stays ours until edge264_return_frame
                n += 1
                cur = Edge264Frame()
                C.memmove(C.byref(cur), C.byref(out), C.sizeof(Edge264Frame))
                assert bool(cur.samples_mvc[0]) == (n_views == 2)
                if kept:
                    views = []
                    for v in range(n_views):
                        rec = np.full(3, 7, backend.DIFF_DTYPE)
                        assert dlib.e264front_frame_diff(dec, C.byref(cur), v, dec, C.byref(kept[0]), v, rec.ctypes.data) == 0, backend.last_error()
                        views.append(dicts(rec))
                    if n_views == 1:
                        rec = np.full(3, 7, backend.DIFF_DTYPE)
                        assert dlib.e264front_frame_diff(dec, C.byref(cur), 1, dec, C.byref(kept[0]), 0, rec.ctypes.data) == errno.EINVAL  # no second view
                        assert (rec == np.full(3, 7, backend.DIFF_DTYPE)).all()
                    got.append(views)
                    lib.edge264_return_frame(dec, kept[0].return_arg)
                    kept.clear()
                else:  # the first frame against itself
                    rec = np.full(3, 7, backend.DIFF_DTYPE)
                    assert dlib.e264front_frame_diff(dec, C.byref(cur), 0, dec, C.byref(cur), 0, rec.ctypes.data) == 0, backend.last_error()
                    assert dicts(rec) == [ZERO] * 3
                kept.append(cur)
            return n
        nal = lib.edge264_find_start_code(base, end, 0) + 3
        while True:
            nxt = lib.edge264_find_start_code(nal, end, 0) if nal < end else end
            res = lib.edge264_decode_NAL(dec, nal, nxt, None, None)
            n = drain()
            if res == errno.ENOBUFS:
                if n == 0:  # the decoder wants EVERY frame back (the end of a sequence, a change of SPS): the kept one too
                    assert kept, "nothing to fetch and nothing kept"
                    lib.edge264_return_frame(dec, kept[0].return_arg)
                    kept.clear()
                continue
            if res == errno.ENODATA or nal >= end:
                break
            nal = min(nxt + 3, end)
        drain()
        if kept:
            lib.edge264_return_frame(dec, kept[0].return_arg)
        lib.edge264_free(C.byref(dec))
    finally:
        lib.e264front_set_download(1)
    assert len(got) == len(want) == len(frames) - 1
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"frame {i + 1} against frame {i}"
    if name == "crop_longterm_mmco":
        assert frames[0][0].shape != (sums[name]["height_mbs"] * 16, sums[name]["width_mbs"] * 16), "the stream is cropped"


def yuv_frames(path, w, h):
    data = np.fromfile(path, np.uint8)
    fb = w * h * 3 // 2
    assert len(data) % fb == 0
    return [data[j:j + fb] for j in range(0, len(data), fb)]


def planes_of(f, w, h):
    return f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)


def diff_line(prev, cur, w, h):
    out = []
    for p, q in zip(planes_of(cur, w, h), planes_of(prev, w, h)):
        r = DF.diff_plane(p, q)
        out.append("%d %d %d %d %s" % (r["count"], r["sad"], r["sse"], r["max"], "-" if r["first"] == NONE else r["first"]))
    return " ".join(out)


def test_driver_diff_mode(tmp_path):
    """e264_multi --diff DIR --out DIR2 on committed streams decoded at once: every line of s<k>.diff is the record of consecutive frames of s<k>.yuv, whose
    frames are the reference's; a --no-download --digest --diff run writes the same lines, and its digest lines equal those of a run without --diff (holding a
    frame changes no output).  No committed stream changes its picture size mid-stream (tests/golden/streams/reference_md5.json: one size per stream), so
    the `size` line is not reached here."""
    for p in (EXE, FRONT, HIP, FRONT_DIGEST):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["ipb_spatial", "t8x8_scaling", "reorder_weighted", "one_mb", "tall_narrow", "cabac_reorder_longterm"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out_dir, diff_dir, diff2_dir, dig_dir, dig2_dir = (tmp_path / d for d in ("out", "diff", "diff2", "digest", "digest2"))
    for d in (out_dir, diff_dir, diff2_dir, dig_dir, dig2_dir):
        d.mkdir()
    common = [EXE, "--front", FRONT, "--hip", HIP, "--repeat", "2", "--threads", "3"]
    r1 = subprocess.run(common + ["--diff", str(diff_dir), "--out", str(out_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(common + ["--no-download", "--digest", str(dig2_dir), "--diff", str(diff2_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    r3 = subprocess.run(common + ["--no-download", "--digest", str(dig_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r3.returncode == 0, r3.stderr[-2000:]
    s1, s2, s3 = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (r1, r2, r3))
    assert s1["frames"] == s2["frames"] == s3["frames"] == 2 * sum(len(sums[n]["md5"]) for n in names)
    i, differing = 0, 0
    for _ in range(2):
        for n in names:
            assert sums[n]["views"] == 1
            w, h = sums[n]["width_mbs"] * 16, sums[n]["height_mbs"] * 16
            nfr = len(sums[n]["md5"])
            frames = yuv_frames(out_dir / f"s{i}.yuv", w, h)
            assert [hashlib.md5(f.tobytes()).hexdigest() for f in frames] == sums[n]["md5"], f"stream {i} ({n})"
            want = [diff_line(prev, cur, w, h) for prev, cur in zip(frames, frames[1:])]
            differing += sum(not ln.startswith("0 0 0 0 -") for ln in want)
            assert (diff_dir / f"s{i}.diff").read_text().splitlines() == want, f"stream {i} ({n})"
            assert (diff2_dir / f"s{i}.diff").read_text().splitlines() == want, f"stream {i} ({n}), --no-download"
            dig = (dig_dir / f"s{i}.digest").read_text().splitlines()
            assert len(dig) == nfr and (dig2_dir / f"s{i}.digest").read_text().splitlines() == dig, f"stream {i} ({n}): digests with and without --diff"
            want_dig = ["%016x %016x %016x" % tuple(D.plane_digest(p) for p in planes_of(f, w, h)) for f in frames]
            assert dig == want_dig, f"stream {i} ({n})"
            i += 1
    assert differing > 20
    r4 = subprocess.run(common + ["--parse-only", "--diff", str(diff_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r4.returncode == 2 and "--diff" in r4.stderr
