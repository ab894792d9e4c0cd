"""The block statistics kernel on the MI355X (e264hip_frame_blockstat / e264hip_blockstat_batch, include/edge264_hip.h): what ONE picture in HBM looks like, block
by block.

Views: planes of a dozen sizes that put 16-column and block boundaries in every relation (17 x 9, 33 x 65, 64 x 64, 65 x 17, 129 x 33, one column, ...), tight
from an aligned start and padded from byte 5 -- the padding once random and once unlike every sample, so that a pair taken from outside the view shows -- a
cropped view of a larger picture, the padded layouts of tests/layouts.py, for every block size, against blockstat.frame_blockstat of the host copy, bit for bit.
The invariants on the device: against e264hip_frame_hist and against e264hip_frame_blockdiff with a zero picture.  A lone 255 at block corners and at the view's
last column and row, a checkerboard, an all-255 block.  Batches of 1 to 257 pictures, a mixed batch, the bytes of `out` a map does not cover.  Ordering behind a
submission and behind uploads with no wait between.  Every refusal.  The front library on cropped, MVC and 1080p streams with borrowed frames, and the driver's
--blockstat mode.  tests/test_blockstat.py runs the kernel's body on the host first.  Everything is compared for equality."""
import ctypes as C
import errno
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, blockstat as BS, digest as D, packet as P, synth
from tests import layouts as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STREAMS = os.path.join(HERE, "golden", "streams")
EXE = os.path.join(ROOT, "edge264_amd", "e264_multi")
FRONT = os.path.join(ROOT, "edge264_amd", "libedge264_hipfront.so")
HIP = os.path.join(ROOT, "edge264_amd", "libedge264_hip.so")
FRONT_DIGEST = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
KS = (3, 4, 5, 6)
DT = backend.BLOCKSTAT_DTYPE
FIELDS = ("sum", "sumsq", "gh", "gv")


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def geo_of(w, h, layout):
    return dict(width_mbs=w, height_mbs=h, **L.geometry(w, h, layout))


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


def raw_view(sizes, pads, start, gap):
    """three planes of any sizes laid one behind the other in a slot: plane p is sizes[p] = (w, h) samples, rows w + pads[p] bytes apart, the first at byte
    `start`, `gap` bytes between planes; returns the view and the bytes it needs"""
    off, view = start, dict(offset=[], stride=[], width=[], height=[])
    for (w, h), pad in zip(sizes, pads):
        view["offset"].append(off); view["stride"].append(w + pad); view["width"].append(w); view["height"].append(h)
        off += (h - 1) * (w + pad) + w + gap
    return view, off - gap


def planes_rw(view, img):
    return [np.lib.stride_tricks.as_strided(img[o:], shape=(h, w), strides=(s, 1)) for o, s, w, h in zip(view["offset"], view["stride"], view["width"], view["height"])]


def view_mask(view, n):
    """the bytes of a slot image of n bytes that are samples of the view"""
    m = np.zeros(n, bool)
    for p in planes_rw(view, m):
        p[:] = True
    return m


def same(got, want):
    """three maps from the device against three from the host: shapes, dtype and every record"""
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == DT and g.shape == w.shape and (g == w).all(), (g.shape, w.shape, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else None)
    return True


# Y, Cb, Cr of a case: twelve sizes -- below, at and above 16 columns and every block size, a single column, a single row, more rows than columns
SIZE_CASES = [((17, 9), (33, 65), (64, 64)), ((65, 17), (129, 33), (1, 70)), ((8, 8), (16, 16), (15, 7)), ((63, 129), (9, 1), (128, 64))]


@pytest.fixture(scope="module")
def raw_slot(device):
    """a stream whose slot is large enough for every SIZE_CASES view (17 x 5 macroblocks: 32640 bytes and a guard)"""
    a = Slot(device, 17, 5, "tight")
    yield a
    a.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", range(len(SIZE_CASES)))
def test_views_of_many_sizes(device, raw_slot, case, k):
    """the planes tight from an aligned start, then padded by 3 / 16 / 1 bytes per row from byte 5 (another alignment in every row): the device's map is the
    host's.  Each with every byte of the slot random, and with samples of 0 .. 127 and 255 in every byte that is no sample of the view (padding, gaps, guard):
    a pair taken from outside the view would add at least 128"""
    a = raw_slot
    rng = np.random.default_rng(100 * case + k)
    sizes = SIZE_CASES[case]
    for what, (view, n) in (("tight", raw_view(sizes, (0, 0, 0), 16 * case, 0)), ("padded", raw_view(sizes, (3, 16, 1), 5 + case, 3))):
        assert n <= a.bytes and backend.blockstat_check(view, a.bytes, k) == 0
        inside = view_mask(view, a.bytes)
        for unlike in (False, True):
            img = rng.integers(0, 256, a.bytes, dtype=np.uint8)
            if unlike:
                img[inside] &= 0x7f
                img[~inside] = 255
            a.upload(img)
            want = BS.frame_blockstat(view, img, k)
            got = a.st.blockstat(0, view, k)
            assert same(got, want), (case, k, what, unlike)
            assert [m.shape for m in got] == [tuple(reversed(d)) for d in backend.blockstat_dims(view, k)]
            if unlike:  # no pair reaches 128 inside the view: had one been taken from outside, gh or gv would show it
                for m, (w, h) in zip(got, sizes):
                    assert int(m["gh"].sum()) <= 127 * (w - 1) * h and int(m["gv"].sum()) <= 127 * w * (h - 1)


def views_of(w, h, geo):
    """whole; a crop with Cb at an odd byte; a crop to an odd chroma width; the bottom-right 2 x 2 luma / 1 x 1 chroma corner"""
    return [D.frame_view(w, h, geometry=geo), D.frame_view(w, h, crop=(2, 6, 2, 10), geometry=geo), D.frame_view(w, h, crop=(6, 0, 2, 0), geometry=geo),
            D.frame_view(w, h, crop=(w * 16 - 2, 0, h * 16 - 2, 0), geometry=geo)]


PICTURES = [(5, 3, "gaps_wide"), (17, 5, "pad16"), (9, 9, "canvas"), (5, 3, "tight")]


@pytest.mark.parametrize("w,h,layout", PICTURES, ids=[f"{w}x{h}-{la}" for w, h, la in PICTURES])
def test_layouts_and_crops(device, w, h, layout):
    """whole, cropped and corner views of a picture in a padded layout, as a batch of four per block size: the cropped-away samples, the padding and the guard
    are noise; the same samples with other bytes everywhere else give the same maps"""
    rng = np.random.default_rng(w * 1000 + h)
    a = Slot(device, w, h, layout)
    try:
        views = views_of(w, h, a.geo)
        img = L.random_slot(a.geo, rng)
        a.upload(img)
        whole = {}
        for k in KS:
            want = [BS.frame_blockstat(v, img, k) for v in views]
            got = device.blockstat_batch([a.st] * 4, [0] * 4, views, k)
            assert len(got) == 4 and all(same(got[i], want[i]) for i in range(4)), k
            whole[k] = want[0]
        a.upload(L.random_slot(a.geo, rng, samples_from=img))
        for k in (3, 6):
            assert same(a.st.blockstat(0, views[0], k), whole[k]), (k, "padding")
    finally:
        a.close()


def test_cropped_view_of_a_larger_picture(device):
    """the 80 x 48 middle of a 6 x 4-macroblock picture (canvas layout) whose cropped-away samples are noise, starting 10 bytes into a 16-byte vector"""
    rng = np.random.default_rng(64)
    a = Slot(device, 6, 4, "canvas")
    try:
        v = D.frame_view(6, 4, crop=(10, 6, 12, 4), geometry=a.geo)
        assert v["width"] == [80, 40, 40] and v["height"] == [48, 24, 24] and v["offset"][0] % 16 == 10
        img = L.random_slot(a.geo, rng)
        inside = view_mask(v, a.bytes)
        img[inside] &= 0x7f
        img[~inside] = 255  # every byte around the crop: a pair taken from there would add at least 128
        a.upload(img)
        for k in KS:
            got = a.st.blockstat(0, v, k)
            assert same(got, BS.frame_blockstat(v, img, k)), k
            assert int(got[0]["gh"].sum()) <= 127 * 79 * 48 and int(got[0]["gv"].sum()) <= 127 * 80 * 47
    finally:
        a.close()


@pytest.mark.parametrize("layout", ["tight", "pad16"])
def test_invariants_against_hist_and_blockdiff_on_the_device(device, layout):
    """per plane the map's sums of sum and sumsq are the first and second moments of Stream.hist of the same view; the map equals Stream.blockdiff against a
    zero-filled slot in sad and sse, record for record; the sums over the maps at k = 3 .. 6 are equal -- all computed on the device"""
    rng = np.random.default_rng(31)
    a, z = Slot(device, 17, 5, layout), Slot(device, 17, 5, layout)
    try:
        img = L.random_slot(a.geo, rng)
        a.upload(img)
        z.upload(np.zeros(z.bytes, np.uint8))
        val = np.arange(256, dtype=np.uint64)
        for v in views_of(17, 5, a.geo)[:3]:
            bins = a.st.hist(0, v).astype(np.uint64)
            totals = set()
            for k in KS:
                got = a.st.blockstat(0, v, k)
                bd = a.st.blockdiff(0, v, z.st, 0, v, k)
                for p in range(3):
                    assert int(got[p]["sum"].sum(dtype=np.uint64)) == int((val * bins[p]).sum()) and int(got[p]["sumsq"].sum(dtype=np.uint64)) == int((val * val * bins[p]).sum())
                    assert (got[p]["sum"] == bd[p]["sad"]).all() and (got[p]["sumsq"] == bd[p]["sse"]).all()
                    n = BS.counts(v["width"][p], v["height"][p], k)
                    assert (n * got[p]["sumsq"].astype(np.int64) - got[p]["sum"].astype(np.int64) ** 2 >= 0).all()
                totals.add(tuple(int(got[p][f].sum(dtype=np.uint64)) for p in range(3) for f in FIELDS))
            assert len(totals) == 1, totals
    finally:
        a.close()
        z.close()


@pytest.mark.parametrize("k", KS)
def test_lone_255_checkerboard_and_full_block(device, k):
    """Y: zeros with a lone 255 at the four corners of an inner block, at the view's last column, at its last row, in its last and first sample -- the pairs to
    its left and above it land in the NEIGHBOURING blocks where it sits at its block's edge; Cb: a 0 / 255 checkerboard of 2 b + 1 square (the largest gh and
    gv); Cr: one block of 255 (the largest sum and sumsq)"""
    bs = 1 << k
    a = Slot(device, 20, 10, "tight")
    try:
        w, h = 3 * bs + 5, 3 * bs + 3
        view, n = raw_view(((w, h), (2 * bs + 1, 2 * bs + 1), (bs, bs)), (1, 3, 0), 7, 5)
        assert n <= a.bytes
        img = np.full(a.bytes, 0x55, np.uint8)  # (what is no sample: unlike 0 and 255)
        y, cb, cr = planes_rw(view, img)
        yy, xx = np.mgrid[0:2 * bs + 1, 0:2 * bs + 1]
        cb[:] = ((yy + xx) & 1) * 255
        cr[:] = 255
        x0, y0, x1, y1 = bs, bs, 2 * bs - 1, 2 * bs - 1
        for x, yq in [(x0, y0), (x1, y0), (x0, y1), (x1, y1), (w - 1, y0 + 2), (x0 + 2, h - 1), (w - 1, h - 1), (0, 0)]:
            y[:] = 0
            y[yq, x] = 255
            a.upload(img)
            got = a.st.blockstat(0, view, k)
            assert same(got, BS.frame_blockstat(view, img, k)), (k, x, yq)
            want = np.zeros((4, 4), DT)
            want[yq >> k, x >> k]["sum"], want[yq >> k, x >> k]["sumsq"] = 255, 65025
            if x + 1 < w:
                want[yq >> k, x >> k]["gh"] += 255
            if x > 0:
                want[yq >> k, (x - 1) >> k]["gh"] += 255
            if yq + 1 < h:
                want[yq >> k, x >> k]["gv"] += 255
            if yq > 0:
                want[(yq - 1) >> k, x >> k]["gv"] += 255
            assert (got[0] == want).all(), (k, x, yq)
            if (x, yq) == (x0, y0):
                assert tuple(got[0][1, 0]) == (0, 0, 255, 0) and tuple(got[0][0, 1]) == (0, 0, 0, 255) and tuple(got[0][1, 1]) == (255, 65025, 255, 255)
        nb = bs * bs
        assert tuple(got[1][0, 0]) == (255 * (nb // 2), 65025 * (nb // 2), 255 * nb, 255 * nb) and tuple(got[1][2, 2]) == (0, 0, 0, 0)
        assert got[2].shape == (1, 1) and tuple(got[2][0, 0]) == (255 * nb, 65025 * nb, 0, 0)
    finally:
        a.close()


@pytest.fixture(scope="module")
def tiny_streams(device):
    """257 streams of 1 x 1-macroblock pictures, distinct contents"""
    rng = np.random.default_rng(257)
    geo = geo_of(1, 1, "tight")
    view = D.frame_view(1, 1, geometry=geo)
    slots, imgs = [], []
    for _ in range(257):
        s = Slot(device, 1, 1, "tight")
        img = L.random_slot(geo, rng)
        s.upload(img)
        slots.append(s)
        imgs.append(img)
    yield slots, view, imgs
    for s in slots:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_batches_of_small_pictures_and_the_bytes_between_the_maps(device, tiny_streams, n):
    """n pictures in one call at k = 3 (six records per picture) and k = 4 (three), results in call order; with a pitch larger than a map, the bytes of `out`
    between the maps and behind the last keep the pattern written in front"""
    slots, view, imgs = tiny_streams
    sts = [s.st for s in slots[:n]]
    for k in (3, 4):
        want = [BS.frame_blockstat(view, img, k) for img in imgs[:n]]
        got = device.blockstat_batch(sts, [0] * n, [view] * n, k)
        assert len(got) == n and all(same(got[i], want[i]) for i in range(n))
        got = device.blockstat_batch(sts[::-1], [0] * n, [view] * n, k)
        assert all(same(got[i], want[n - 1 - i]) for i in range(n))
        size = backend.blockstat_bytes(view, k)
        assert size == (96 if k == 3 else 48)
        pitch = size + 13
        out = np.full(n * pitch + 32, 0xa5, np.uint8)
        sa = (C.c_void_p * n)(*[s.h for s in sts])
        s0 = (C.c_int * n)(*[0] * n)
        cv = (backend.View * n)(*[backend.as_view(view)] * n)
        assert device.L.e264hip_blockstat_batch(device.h, sa, s0, cv, n, k, out.ctypes.data, pitch) == 0, backend.last_error()
        rows = out[:n * pitch].reshape(n, pitch)
        assert (rows[:, size:] == 0xa5).all() and (out[n * pitch:] == 0xa5).all()
        for i in range(n):
            flat = np.concatenate([m.reshape(-1) for m in want[i]])
            assert (rows[i, :size].copy().view(DT) == flat).all(), i


def test_mixed_batch(device):
    """pictures of four sizes in one call, each stream in its own layout, a stream appearing more than once, whole and cropped views"""
    rng = np.random.default_rng(77)
    sizes = [(1, 1), (5, 3), (17, 5), (130, 5)]
    slots = [Slot(device, *sizes[i % 4], L.MIXED[i % len(L.MIXED)]) for i in range(8)]
    try:
        imgs = []
        for s in slots:
            img = L.random_slot(s.geo, rng)
            s.upload(img)
            imgs.append(img)
        who, views = [], []
        for i, s in enumerate(slots):
            for j in (0, 1, 2, 3, 0):
                who.append(i); views.append(views_of(s.w, s.h, s.geo)[j])
        for k in KS:
            got = device.blockstat_batch([slots[i].st for i in who], [0] * len(who), views, k)
            assert len(got) == 40
            for j in range(40):
                assert same(got[j], BS.frame_blockstat(views[j], imgs[who[j]], k)), (k, j)
    finally:
        for s in slots:
            s.close()


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


@pytest.mark.parametrize("lane", [0, 2])
def test_ordering_behind_a_submission(device, oracle, lane):
    """the packet submitted, the map asked for with nothing between: the map of the oracle's picture, for I, P and B; then a batch of three streams behind
    submit_batch_host"""
    st, dpb, nb = open_smoke_stream(device, lane)
    sts = [open_smoke_stream(device, lane) for _ in range(3)]
    try:
        view = D.frame_view(8, 6)
        gen = smoke_gop()
        for t, k in zip("IPB", (4, 3, 5)):
            pkt = gen.next_frame(t)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            oracle.decode_frame(pkt, dpb, 3)
            st.submit(pkt)
            assert same(st.blockstat(d, view, k), BS.frame_blockstat(view, dpb[d][:nb], k)), t
        gens = [smoke_gop(seed) for seed in (1, 2, 3)]
        for t in "IPB":
            pkts = [g.next_frame(t) for g in gens]
            dst = [int(P.Packet(p).hdr["dst_slot"]) for p in pkts]
            for j, (_, dpb_j, _) in enumerate(sts):
                oracle.decode_frame(pkts[j], dpb_j, 3)
            device.submit_batch_host([s[0] for s in sts], pkts)
            got = device.blockstat_batch([s[0] for s in sts], dst, [view] * 3, 4)
            for j, (_, dpb_j, nb_j) in enumerate(sts):
                assert same(got[j], BS.frame_blockstat(view, dpb_j[dst[j]][:nb_j], 4)), (t, j)
    finally:
        st.close()
        for s in sts:
            s[0].close()


@pytest.mark.parametrize("lane", [0, 1])
def test_ordering_behind_host_uploads_on_the_same_lane(device, lane):
    """upload, map, upload, map ... with no wait between: every map is that of the picture uploaded just in front of it, never of the one before"""
    rng = np.random.default_rng(12 + lane)
    a = Slot(device, 17, 5, "pad16", lane=lane)
    try:
        v = views_of(17, 5, a.geo)[1]
        imgs = [L.random_slot(a.geo, rng) for _ in range(6)]
        for i, img in enumerate(imgs):
            a.upload(img)
            assert same(a.st.blockstat(0, v, KS[i % 4]), BS.frame_blockstat(v, img, KS[i % 4])), i
    finally:
        a.close()


def test_errors(device):
    """every refusal is EINVAL with a text, leaves `out` untouched and queues nothing: a valid call right after it gives the right map"""
    lib = device.L
    rng = np.random.default_rng(9)
    a, other_lane, small = Slot(device, 5, 3, "pad16"), Slot(device, 5, 3, "pad16", lane=1), Slot(device, 1, 1, "tight")
    large = Slot(device, 64, 32, "tight")  # 1024 x 512: a map of 196608 bytes at k = 3
    dev2 = backend.Device(0)  # a second device object: its streams are not `device`'s
    foreign = Slot(dev2, 5, 3, "pad16")
    try:
        img_a = L.random_slot(a.geo, rng)
        a.upload(img_a)
        other_lane.upload(img_a)
        foreign.upload(img_a)
        small.upload(L.random_slot(small.geo, rng))
        va = views_of(5, 3, a.geo)[1]
        want = BS.frame_blockstat(va, img_a, 4)
        size = backend.blockstat_bytes(va, 4)
        ca = backend.as_view(va)
        out = np.full(2 * size + 64, 7, np.uint8)
        clone = backend.View.from_buffer_copy  # (as_view hands a View back as it is: a changed copy must not change the good one)

        def call(dev=device.h, streams=(a.st.h,), slots=(0,), views=(ca,), n=None, k=4, res=out.ctypes.data, pitch=size):
            m = len(streams) if streams is not None else 1
            arr = lambda t, x: (t * len(x))(*x) if x is not None else None
            return lib.e264hip_blockstat_batch(dev, arr(C.c_void_p, streams), arr(C.c_int, slots), arr(backend.View, views), m if n is None else n, k, res, pitch)

        def refused(what, **kw):
            assert call(**kw) == errno.EINVAL, what
            assert backend.last_error(), what
            assert (out == 7).all(), what
            assert same(a.st.blockstat(0, va, 4), want), f"after the refusal of {what}"

        refused("a null device", dev=None)
        for name in ("streams", "slots", "views"):
            refused("null " + name, **{name: None})
        refused("null out", res=None)
        refused("a null stream", streams=(None,))
        refused("n < 0", n=-1)
        refused("n > 4096", n=4097)
        for k in (-1, 0, 2, 7):
            refused(f"k = {k}", k=k)
            assert "log2_block" in backend.last_error()
        refused("slot -1", slots=(-1,))
        refused("a slot past the table", slots=(P.MAX_SLOTS,))
        refused("a slot that is not allocated", slots=(5,))
        refused("streams of two lanes", streams=(a.st.h, other_lane.st.h), slots=(0, 0), views=(ca, ca))
        refused("a stream of another device", streams=(foreign.st.h,))
        bad = clone(ca)
        bad.plane[2].height += 4096
        refused("a view that leaves the slot", views=(bad,))
        bad = clone(ca)
        bad.plane[1].width = 0
        refused("a plane without samples", views=(bad,))
        refused("the second picture's view", streams=(a.st.h, a.st.h), slots=(0, 0), views=(ca, bad))
        bad = clone(ca)
        bad.plane[0].stride = bad.plane[0].width - 1
        refused("a stride below the width", views=(bad,))
        refused("a view valid for a larger slot, not for this one", streams=(small.st.h,), views=(backend.as_view(D.frame_view(5, 3)),))
        # pitch and cap
        refused("a pitch one byte short", pitch=size - 1)
        assert "pitch" in backend.last_error()
        refused("a pitch of 0", pitch=0)
        vs = backend.as_view(D.frame_view(1, 1, geometry=small.geo))
        refused("the second picture's map larger than the pitch", streams=(small.st.h, a.st.h), slots=(0, 0), views=(vs, ca), pitch=size - 16)
        o = out.ctypes.data
        assert lib.e264hip_frame_blockstat(a.st.h, 0, C.byref(ca), 4, o, size - 1) == errno.EINVAL and "cap" in backend.last_error()
        # more than E264_BLOCKSTAT_MAX_BYTES in one call: 4096 maps of 196608 bytes
        vl = backend.as_view(D.frame_view(64, 32, geometry=large.geo))
        big = backend.blockstat_bytes(vl, 3)
        assert big == 196608 and 4096 * big > backend.BLOCKSTAT_MAX_BYTES >= 1365 * big
        refused("more than E264_BLOCKSTAT_MAX_BYTES", streams=(large.st.h,) * 4096, slots=(0,) * 4096, views=(vl,) * 4096, k=3, pitch=big)
        assert "E264_BLOCKSTAT_MAX_BYTES" in backend.last_error()
        # frame_blockstat, the batch of one
        assert lib.e264hip_frame_blockstat(None, 0, C.byref(ca), 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockstat(a.st.h, 0, None, 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockstat(a.st.h, 0, C.byref(ca), 4, None, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockstat(a.st.h, 7, C.byref(ca), 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockstat(a.st.h, 0, C.byref(ca), 9, o, size) == errno.EINVAL and backend.last_error()
        with pytest.raises(ValueError):
            a.st.blockstat(0, va, 2)
        with pytest.raises(ValueError):
            device.blockstat_batch([a.st], [0], [], 4)
        # n == 0 is no error, with or without arrays
        assert call(n=0) == 0 and call(streams=None, slots=None, views=None, n=0, res=None, pitch=0) == 0
        assert device.blockstat_batch([], [], [], 4) == []
        assert (out == 7).all()  # no call above wrote anything
        # a cap larger than the map: only the map's bytes are written
        assert lib.e264hip_frame_blockstat(a.st.h, 0, C.byref(ca), 4, o, out.nbytes) == 0
        assert (out[:size].copy().view(DT) == np.concatenate([m.reshape(-1) for m in want])).all() and (out[size:] == 7).all()
        assert same(other_lane.st.blockstat(0, va, 4), want)  # (the stream of the other lane)
        assert same(foreign.st.blockstat(0, va, 4), want)     # (... and of the other device object)
    finally:
        for s in (a, other_lane, small, large, foreign):
            s.close()
        dev2.close()


class CBlockStat(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in FIELDS]


@pytest.fixture(scope="module")
def c_header(tmp_path_factory):
    """include/edge264_blockstat.h's e264_blockstat_plane in a temporary library: what the front library's maps are compared with"""
    if not shutil.which("gcc"):
        pytest.fail("no gcc")
    d = tmp_path_factory.mktemp("blockstat_c")
    src = d / "bs.c"
    src.write_text('#include "edge264_blockstat.h"\n'
                   'void bs_plane(const unsigned char *s, unsigned long stride, unsigned w, unsigned h, int k, E264BlockStat *out) { e264_blockstat_plane(s, stride, w, h, k, out); }\n')
    lib = d / "libbs.so"
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(lib)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lc = C.CDLL(str(lib))
    lc.bs_plane.restype = None
    lc.bs_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_uint, C.c_int, C.c_void_p]

    def plane(a, k):
        a = np.ascontiguousarray(a)
        bw, bh = BS.blockstat_dims(a.shape[1], a.shape[0], k)
        out = np.zeros((bh, bw), DT)
        lc.bs_plane(a.ctypes.data, a.strides[0], a.shape[1], a.shape[0], k, out.ctypes.data)
        return out
    return plane


def md5s(frames):
    return [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames]


@pytest.mark.parametrize("download", [1, 0], ids=["download", "no-download"])
@pytest.mark.parametrize("name", ["crop_longterm_mmco", "mvc_ipp", "hd1080_ippb"])
def test_front_end(c_header, name, download):
    """e264front_frame_blockstat over the output frames fetched with borrow = 1 (returned after the call), with read-back on and off, equals
    include/edge264_blockstat.h's e264_blockstat_plane over the planes a second, downloading decoder delivered, which are the reference's; the block size goes
    round 3 .. 6"""
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
    ks = [KS[i % 4] for i in range(len(frames))]
    want = [[[c_header(p, k) for p in fr[3 * v:3 * v + 3]] for v in range(n_views)] for fr, k in zip(frames, ks)]
    assert (want[0][0][0] == BS.plane_blockstat(frames[0][0], ks[0])).all()
    assert os.path.exists(FRONT_DIGEST), f"{FRONT_DIGEST} missing (built by __graft_entry__.build() on every machine)"
    dlib = C.CDLL(FRONT_DIGEST)  # e264front_frame_blockstat: edge264_amd/frontend/front_blockstat.c, in the library beside the front library
    fn = dlib.e264front_frame_blockstat
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint16)]
    buf = np.frombuffer(data + b"\0" * 64, np.uint8).copy()
    base, end = buf.ctypes.data, buf.ctypes.data + len(data)
    got = []
    cap = 16 * (3 * (-(-frames[0][0].shape[1] // 8)) * (-(-frames[0][0].shape[0] // 8)))  # more than any map of these frames
    lib.e264front_set_download(download)
    try:
        dec = C.c_void_p(lib.edge264_alloc(0, None, None, 0, None, None, None))
        assert dec
        out = Edge264Frame()

        def one(cur, v, k):
            raw = np.full(cap, 7, np.uint8)
            dims = (C.c_uint16 * 6)()
            r = fn(dec, C.byref(cur), v, k, raw.ctypes.data, cap, dims)
            if r:
                assert (raw == 7).all()
                return r
            d = [(int(dims[2 * p]), int(dims[2 * p + 1])) for p in range(3)]
            size = 16 * sum(bw * bh for bw, bh in d)
            assert (raw[size:] == 7).all()
            return BS.split_map(raw, d)

        def drain():
            n = 0
            while lib.edge264_get_frame(dec, C.byref(out), 1) == 0:  # borrowed: the frame stays ours until edge264_return_frame
                n += 1
                assert bool(out.samples_mvc[0]) == (n_views == 2)
                k = ks[len(got)]
                got.append([one(out, v, k) for v in range(n_views)])
                if n_views == 1:
                    assert one(out, 1, k) == errno.EINVAL  # no second view
                small = np.full(16, 7, np.uint8)
                assert fn(dec, C.byref(out), 0, k, small.ctypes.data, 15, None) == errno.EINVAL and (small == 7).all()  # cap smaller than the map
                lib.edge264_return_frame(dec, out.return_arg)
            return n
        nal = lib.edge264_find_start_code(base, end, 0) + 3
        while True:
            nxt = lib.edge264_find_start_code(nal, end, 0) if nal < end else end
            res = lib.edge264_decode_NAL(dec, nal, nxt, None, None)
            drain()
            if res == errno.ENOBUFS:
                continue
            if res == errno.ENODATA or nal >= end:
                break
            nal = min(nxt + 3, end)
        drain()
        lib.edge264_free(C.byref(dec))
    finally:
        lib.e264front_set_download(1)
    assert len(got) == len(want) == len(frames)
    for i, (g, w) in enumerate(zip(got, want)):
        for v in range(n_views):
            assert same(g[v], w[v]), f"frame {i}, view {v}, k {ks[i]}"
    if name == "crop_longterm_mmco":
        assert frames[0][0].shape != (sums[name]["height_mbs"] * 16, sums[name]["width_mbs"] * 16), "the stream is cropped"


def yuv_frames(path, w, h):
    data = np.fromfile(path, np.uint8)
    fb = w * h * 3 // 2
    assert len(data) % fb == 0
    return [data[j:j + fb] for j in range(0, len(data), fb)]


def planes_of(f, w, h):
    return f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)


def parse_blockstat_file(path):
    """the records of s<k>.blockstat: [(k, [(bw, bh)] * 3, [Y, Cb, Cr maps])]"""
    data, at, out = open(path, "rb").read(), 0, []
    while at < len(data):
        d = struct.unpack_from("<6HI", data, at)
        at += 16
        dims, k = [(d[0], d[1]), (d[2], d[3]), (d[4], d[5])], d[6]
        size = 16 * sum(bw * bh for bw, bh in dims)
        assert at + size <= len(data)
        out.append((k, dims, BS.split_map(np.frombuffer(data, np.uint8, size, at), dims)))
        at += size
    return out


def test_driver_blockstat_mode(tmp_path):
    """e264_multi --blockstat DIR --out DIR2 on two committed streams: every record of s<k>.blockstat is the header and the map of the frame of s<k>.yuv, whose
    frames are the reference's, at the default block size, from the first frame on; --no-download --blockstat-log2 3 writes the maps at 8 x 8; refused with
    --parse-only and for a block size outside 3..6 (exit status 2); without the flag the driver writes the same pictures, byte for byte (the --out files with and without --blockstat
    are compared with each other and, by md5, with the reference's pictures, which the parent writes too; the parent's own binary is not run here)"""
    for p in (EXE, FRONT, HIP, FRONT_DIGEST):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["ipb_spatial", "tall_narrow"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out_dir, out0_dir, bs_dir, bs2_dir = (tmp_path / d for d in ("out", "out0", "bs", "bs2"))
    for d in (out_dir, out0_dir, bs_dir, bs2_dir):
        d.mkdir()
    common = [EXE, "--front", FRONT, "--hip", HIP, "--threads", "2"]
    r1 = subprocess.run(common + ["--blockstat", str(bs_dir), "--out", str(out_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(common + ["--no-download", "--blockstat", str(bs2_dir), "--blockstat-log2", "3"] + files, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    r0 = subprocess.run(common + ["--out", str(out0_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0, r0.stderr[-2000:]
    s1, s2, s0 = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (r1, r2, r0))
    assert s1["frames"] == s2["frames"] == s0["frames"] == sum(len(sums[n]["md5"]) for n in names)
    for i, n in enumerate(names):
        assert sums[n]["views"] == 1
        w, h = sums[n]["width_mbs"] * 16, sums[n]["height_mbs"] * 16
        frames = yuv_frames(out_dir / f"s{i}.yuv", w, h)
        assert [hashlib.md5(f.tobytes()).hexdigest() for f in frames] == sums[n]["md5"], f"stream {i} ({n})"
        assert (out0_dir / f"s{i}.yuv").read_bytes() == (out_dir / f"s{i}.yuv").read_bytes(), f"stream {i} ({n}): --out with and without --blockstat"
        assert sorted(os.listdir(out0_dir)) == sorted(os.listdir(out_dir))
        for d, k in ((bs_dir, 4), (bs2_dir, 3)):
            recs = parse_blockstat_file(d / f"s{i}.blockstat")
            assert len(recs) == len(frames)
            for j, (rk, dims, maps) in enumerate(recs):
                planes = planes_of(frames[j], w, h)
                assert rk == k and dims == [BS.blockstat_dims(p.shape[1], p.shape[0], k) for p in planes]
                assert same(maps, [BS.plane_blockstat(p, k) for p in planes]), (n, j, k)
    r4 = subprocess.run(common + ["--parse-only", "--blockstat", str(bs_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r4.returncode == 2 and "--blockstat" in r4.stderr
    r5 = subprocess.run(common + ["--blockstat", str(bs_dir), "--blockstat-log2", "7"] + files, capture_output=True, text=True, timeout=600)
    assert r5.returncode == 2 and "--blockstat-log2" in r5.stderr
