"""The block difference kernel on the MI355X (e264hip_frame_blockdiff / e264hip_blockdiff_batch, include/edge264_hip.h): WHERE two pictures in HBM differ.

Views: planes of a dozen sizes that put 16-column and block boundaries in every relation (17 x 9, 33 x 65, 64 x 64, 65 x 17, 129 x 33, one column, ...), A tight
and B padded at other alignments, a cropped view against an uncropped picture, the padded layouts of tests/layouts.py, for every block size, against
blockdiff.frame_blockdiff of the host copies, bit for bit, and the sums against e264hip_frame_diff of the same pair on the device.  Single changed samples at block
corners, at the view's last column and row, in each plane.  0 against 255 in a 64 x 64 block.  A picture against itself.  The bytes of `out` a map does not cover.
Batches of 1 to 257 pairs, a mixed batch.  Ordering behind a submission and a host batch with no wait between.  Every refusal.  The front library on cropped, MVC
and 1080p streams with borrowed frames, and the driver's --blockdiff mode.  tests/test_blockdiff.py runs the kernel's body on the host first."""
import ctypes as C
import errno
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, blockdiff as BD, diff as DF, digest as D, packet as P, synth
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
DT = backend.BLOCKDIFF_DTYPE


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


def same(got, want):
    """three maps from the device against three from the host: shapes, dtype and every record"""
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == DT and g.shape == w.shape and (g == w).all(), (g.shape, w.shape, np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else None)
    return True


def sums_match(maps, rec):
    """the sum invariant: a plane's records add up to the difference record's sad and sse of the same pair"""
    for p in range(3):
        assert int(maps[p]["sad"].sum(dtype=np.uint64)) == int(rec[p]["sad"]) and int(maps[p]["sse"].sum(dtype=np.uint64)) == int(rec[p]["sse"]), p
        assert ((maps[p]["sad"] == 0) == (maps[p]["sse"] == 0)).all()
    return True


# Y, Cb, Cr of a case: twelve sizes -- below, at and above 16 columns and every block size, a single column, a single row, more rows than columns
SIZE_CASES = [((17, 9), (33, 65), (64, 64)), ((65, 17), (129, 33), (1, 70)), ((8, 8), (16, 16), (15, 7)), ((63, 129), (9, 1), (128, 64))]


@pytest.fixture(scope="module")
def raw_slots(device):
    """two streams whose slots are large enough for every SIZE_CASES view (17 x 5 macroblocks: 32640 bytes and more), A tight and B pad16"""
    a, b = Slot(device, 17, 5, "tight"), Slot(device, 17, 5, "pad16")
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", range(len(SIZE_CASES)))
def test_views_of_many_sizes(device, raw_slots, case, k):
    """A's planes tight from an aligned start, B's padded by 3 / 16 / 1 bytes per row from byte 5 (other alignments in every row): the device's map is the
    host's, for B = A but for some samples (most blocks equal) and for two unrelated pictures (every vector differs); the sums are e264hip_frame_diff's"""
    a, b = raw_slots
    rng = np.random.default_rng(100 * case + k)
    sizes = SIZE_CASES[case]
    va, na = raw_view(sizes, (0, 0, 0), 16 * case, 0)
    vb, nb = raw_view(sizes, (3, 16, 1), 5 + case, 3)
    assert na <= a.bytes and nb <= b.bytes and backend.blockdiff_check(va, a.bytes, vb, b.bytes, k) == 0
    img_a = rng.integers(0, 256, a.bytes, dtype=np.uint8)
    a.upload(img_a)
    for unrelated in (False, True):
        img_b = rng.integers(0, 256, b.bytes, dtype=np.uint8)
        if not unrelated:
            for pa, pb in zip(planes_rw(va, img_a), planes_rw(vb, img_b)):
                pb[:] = pa
                h, w = pb.shape
                for _ in range(1 + w * h // 200):
                    pb[int(rng.integers(0, h)), int(rng.integers(0, w))] ^= int(rng.integers(1, 256))
                pb[h - 1, w - 1] ^= 0x40  # the view's last sample
        b.upload(img_b)
        want = BD.frame_blockdiff(va, img_a, vb, img_b, k)
        got = a.st.blockdiff(0, va, b.st, 0, vb, k)
        assert same(got, want), (case, k, unrelated)
        assert [m.shape for m in got] == [tuple(reversed(d)) for d in backend.blockdiff_dims(va, k)]
        assert sums_match(got, a.st.diff(0, va, b.st, 0, vb))
        # the other way round gives the same map (|a - b| is symmetric)
        assert same(b.st.blockdiff(0, vb, a.st, 0, va, k), want)


def views_of(w, h, geo):
    """whole; a crop with Cb at an odd byte; a crop to an odd chroma width; the bottom-right 2 x 2 luma / 1 x 1 chroma corner"""
    return [D.frame_view(w, h, geometry=geo), D.frame_view(w, h, crop=(2, 6, 2, 10), geometry=geo), D.frame_view(w, h, crop=(6, 0, 2, 0), geometry=geo),
            D.frame_view(w, h, crop=(w * 16 - 2, 0, h * 16 - 2, 0), geometry=geo)]


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
    L.samples(geo_b, b)[0][:] = ya
    W, H = geo_b["width_mbs"] * 16, geo_b["height_mbs"] * 16
    sc, psy = geo_b["stride_C"], geo_b["plane_size_Y"]
    c = b[psy:psy + sc * (H // 2)].reshape(H // 2, sc)
    c[:, :W // 2] = ca[:, :W // 2]
    c[:, sc // 2:sc // 2 + W // 2] = ca[:, W // 2:]
    return b


PICTURES = [(5, 3, "tight", "gaps_wide"), (17, 5, "pad16", "canvas"), (9, 9, "canvas", "tight")]


@pytest.mark.parametrize("w,h,la,lb", PICTURES, ids=[f"{w}x{h}-{la}-{lb}" for w, h, la, lb in PICTURES])
def test_layouts_and_crops(device, w, h, la, lb):
    """whole, cropped and corner views of pictures in two different padded layouts and streams, as a batch of four per block size; the same samples with other
    bytes in the padding give the same maps"""
    rng = np.random.default_rng(w * 1000 + h)
    a, b = Slot(device, w, h, la), Slot(device, w, h, lb)
    try:
        va, vb = views_of(w, h, a.geo), views_of(w, h, b.geo)
        img_a = L.random_slot(a.geo, rng)
        img_b = in_layout(img_a, a.geo, b.geo, rng)
        for p in range(3):
            n = (w * 16 >> (p > 0)) * (h * 16 >> (p > 0))
            for i in list(rng.integers(0, n, 9)) + [n - 1]:
                img_b[plane_index(b.geo, p, int(i))] ^= int(rng.integers(1, 256))
        a.upload(img_a)
        b.upload(img_b)
        img_a2, img_b2 = L.random_slot(a.geo, rng, samples_from=img_a), L.random_slot(b.geo, rng, samples_from=img_b)
        for k in KS:
            want = [BD.frame_blockdiff(x, img_a, y, img_b, k) for x, y in zip(va, vb)]
            assert all(BD.changed(m).any() for m in want[0]) and (k > 3 or not any(BD.changed(m).all() for m in want[0]))
            got = device.blockdiff_batch([a.st] * 4, [0] * 4, va, [b.st] * 4, [0] * 4, vb, k)
            assert len(got) == 4 and all(same(got[i], want[i]) for i in range(4)), k
        a.upload(img_a2)
        b.upload(img_b2)
        for k in (3, 6):
            got = device.blockdiff_batch([a.st] * 4, [0] * 4, va, [b.st] * 4, [0] * 4, vb, k)
            assert all(same(got[i], BD.frame_blockdiff(va[i], img_a, vb[i], img_b, k)) for i in range(4)), (k, "padding")
    finally:
        a.close()
        b.close()


def test_cropped_against_uncropped(device):
    """the 80 x 48 middle of a 6 x 4-macroblock picture (canvas layout) against a whole 5 x 3-macroblock picture (tight): two slot sizes, two strides, one view size"""
    rng = np.random.default_rng(64)
    a, b = Slot(device, 6, 4, "canvas"), Slot(device, 5, 3, "tight")
    try:
        va, vb = D.frame_view(6, 4, crop=(10, 6, 12, 4), geometry=a.geo), D.frame_view(5, 3, geometry=b.geo)
        assert va["width"] == vb["width"] == [80, 40, 40] and va["height"] == vb["height"] == [48, 24, 24] and va["offset"][0] % 16 == 10
        img_a, img_b = L.random_slot(a.geo, rng), L.random_slot(b.geo, rng)
        for pa, pb in zip(planes_rw(va, img_a), planes_rw(vb, img_b)):
            pb[:] = pa
            pb[::7, ::13] ^= 0x21
        a.upload(img_a)
        b.upload(img_b)
        for k in KS:
            got = a.st.blockdiff(0, va, b.st, 0, vb, k)
            assert same(got, BD.frame_blockdiff(va, img_a, vb, img_b, k)) and sums_match(got, a.st.diff(0, va, b.st, 0, vb)), k
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("k", KS)
def test_single_changed_samples(device, k):
    """17 x 5 macroblocks cropped to 266 x 78 (chroma 133 x 39: partial blocks at the right and the bottom for every block size), pad16 against tight: one sample
    changed by 3 at each corner of an inner block, at the view's last column and last row and in the corner block gives exactly one record (3, 9), in each plane"""
    rng = np.random.default_rng(175 + k)
    w, h, bs = 17, 5, 1 << k
    a, b = Slot(device, w, h, "pad16"), Slot(device, w, h, "tight")
    try:
        va, vb = D.frame_view(w, h, crop=(0, 6, 0, 2), geometry=a.geo), D.frame_view(w, h, crop=(0, 6, 0, 2), geometry=b.geo)
        img_a = L.random_slot(a.geo, rng)
        m = L.sample_mask(a.geo)
        img_a[m] = np.clip(img_a[m], 3, 252)  # every sample can move by 3 either way
        base_b = in_layout(img_a, a.geo, b.geo, rng)
        a.upload(img_a)
        b.upload(base_b)
        dims = backend.blockdiff_dims(va, k)
        assert not any(BD.changed(x).any() for x in a.st.blockdiff(0, va, b.st, 0, vb, k))
        for p in range(3):
            W, H = va["width"][p], va["height"][p]
            bw, bh = dims[p]
            X, Y = min(1, bw - 1), 0  # an inner block where there is one (at b = 64 chroma has a single row of blocks)
            x0, y0, x1, y1 = bs * X, bs * Y, min(bs * X + bs, W) - 1, min(bs * Y + bs, H) - 1
            spots = [(x0, y0), (x1, y0), (x0, y1), (x1, y1), (W - 1, H // 2), (W // 2, H - 1), (W - 1, H - 1)]
            assert W % bs and H % bs  # the last column and row lie in partial blocks
            for i, (x, y) in enumerate(spots):
                img_b = base_b.copy()
                at = vb["offset"][p] + y * vb["stride"][p] + x
                img_b[at] = int(img_b[at]) + (3 if i & 1 else -3)
                b.upload(img_b)
                got = a.st.blockdiff(0, va, b.st, 0, vb, k)
                want = [np.zeros((dims[q][1], dims[q][0]), DT) for q in range(3)]
                want[p][y >> k, x >> k] = (3, 9)
                assert same(got, want), (p, x, y)
    finally:
        a.close()
        b.close()


def test_extremes_and_the_same_picture(device):
    """one 64 x 64 block of 0 against 255 at k = 6 is the largest record there is (sad 4096 * 255, sse 4096 * 255^2 < 2^32), and the smaller blocks share it out;
    the same slot and view on both sides gives zeros everywhere; Stream.blockdiff's defaults"""
    a, b = backend.Stream(device, 4, 4), backend.Stream(device, 4, 4)
    try:
        for s, v in ((a, 0), (b, 255)):
            s.alloc(0)
            s.fill(0, v)
        for k in KS:
            n = 1 << 2 * k
            for x, y in ((a, b), (b, a)):
                got = x.blockdiff(0, other=y, k=k)
                c = max(32 >> k, 1)
                assert [m.shape for m in got] == [(64 >> k, 64 >> k), (c, c), (c, c)]
                assert (got[0]["sad"] == 255 * n).all() and (got[0]["sse"] == 65025 * n).all()
                nc = min(n, 1024)
                assert (got[1]["sad"] == 255 * nc).all() and (got[2]["sse"] == 65025 * nc).all()
        big = a.blockdiff(0, other=b, k=6)[0]
        assert big.shape == (1, 1) and int(big[0, 0]["sad"]) == 4096 * 255 and int(big[0, 0]["sse"]) == 4096 * 65025 == 266342400
        rng = np.random.default_rng(5)
        img = rng.integers(0, 256, a.frame_bytes, dtype=np.uint8)
        a.upload(0, img)
        v = D.frame_view(4, 4)
        b.alloc(1)
        b.upload(1, img[::-1].copy())
        for k in KS:
            got = a.blockdiff(0, k=k)  # the same stream, slot and view
            assert all(not m["sad"].any() and not m["sse"].any() for m in got)
            assert same(a.blockdiff(0, other=b, other_slot=1, k=k), BD.frame_blockdiff(v, img, v, img[::-1].copy(), k))
    finally:
        a.close()
        b.close()


@pytest.fixture(scope="module")
def tiny_streams(device):
    """257 streams of 1 x 1-macroblock pictures with two slots each, distinct contents; every fourth pair is equal"""
    rng = np.random.default_rng(257)
    geo = geo_of(1, 1, "tight")
    view = D.frame_view(1, 1, geometry=geo)
    slots, imgs = [], []
    for k in range(257):
        s = Slot(device, 1, 1, "tight", n_slots=2)
        img0 = L.random_slot(geo, rng)
        img1 = img0.copy() if k % 4 == 0 else L.random_slot(geo, rng, samples_from=img0)
        for _ in range(k % 4):
            img1[int(rng.integers(0, 384))] ^= int(rng.integers(1, 256))
        s.upload(img0, 0)
        s.upload(img1, 1)
        slots.append(s)
        imgs.append((img0, img1))
    yield slots, view, imgs
    for s in slots:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_batches_of_small_pictures_and_the_bytes_between_the_maps(device, tiny_streams, n):
    """n pairs in one call at k = 3 (six records per pair) and k = 4 (three), results in call order; with a pitch larger than a map, the bytes of `out` between
    the maps and behind the last keep the caller's sentinel"""
    slots, view, imgs = tiny_streams
    sts = [s.st for s in slots[:n]]
    for k in (3, 4):
        want = [BD.frame_blockdiff(view, i0, view, i1, k) for i0, i1 in imgs[:n]]
        got = device.blockdiff_batch(sts, [0] * n, [view] * n, sts, [1] * n, [view] * n, k)
        assert len(got) == n and all(same(got[i], want[i]) for i in range(n))
        got = device.blockdiff_batch(sts[::-1], [0] * n, [view] * n, sts[::-1], [1] * n, [view] * n, k)
        assert all(same(got[i], want[n - 1 - i]) for i in range(n))
        # the C entry point with a pitch of its own
        size = backend.blockdiff_bytes(view, k)
        assert size == (48 if k == 3 else 24)
        pitch = size + 13
        out = np.full(n * pitch + 32, 0xa5, np.uint8)
        sa = (C.c_void_p * n)(*[s.h for s in sts])
        s0, s1 = (C.c_int * n)(*[0] * n), (C.c_int * n)(*[1] * n)
        cv = (backend.View * n)(*[backend.as_view(view)] * n)
        assert device.L.e264hip_blockdiff_batch(device.h, sa, s0, cv, sa, s1, cv, n, k, out.ctypes.data, pitch) == 0, backend.last_error()
        rows = out[:n * pitch].reshape(n, pitch)
        assert (rows[:, size:] == 0xa5).all() and (out[n * pitch:] == 0xa5).all()
        for i in range(n):
            flat = np.concatenate([m.reshape(-1) for m in want[i]])
            assert (rows[i, :size].copy().view(DT) == flat).all(), i


def test_mixed_batch(device):
    """pairs of four sizes in one call, each stream in its own layout, a stream appearing on both sides and more than once, equal and unequal pairs
    interleaved, whole and cropped views"""
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
            for j in range(3):
                sa.append(x); sb.append(y); va.append(views_of(x.w, x.h, x.geo)[j]); vb.append(views_of(y.w, y.h, y.geo)[j]); ia.append(i); ib.append(i + 4)
            sa.append(y); sb.append(x); va.append(views_of(y.w, y.h, y.geo)[0]); vb.append(views_of(x.w, x.h, x.geo)[0]); ia.append(i + 4); ib.append(i)
            sa.append(x); sb.append(x); va.append(views_of(x.w, x.h, x.geo)[1]); vb.append(views_of(x.w, x.h, x.geo)[1]); ia.append(i); ib.append(i)
        for k in KS:
            got = device.blockdiff_batch([s.st for s in sa], [0] * len(sa), va, [s.st for s in sb], [0] * len(sb), vb, k)
            assert len(got) == 20
            for j in range(20):
                assert same(got[j], BD.frame_blockdiff(va[j], imgs[ia[j]], vb[j], imgs[ib[j]], k)), (k, j)
            assert not any(BD.changed(m).any() for m in got[0]) and all(BD.changed(m).any() for m in got[5]) and not any(BD.changed(m).any() for m in got[4])
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


def open_plain_stream(dev, lane=0):
    st = backend.Stream(dev, 8, 6)
    if lane:
        st.bind_lane(lane)
    st.alloc(0)
    return st


def all_zero(maps):
    return all(not m["sad"].any() and not m["sse"].any() for m in maps)


@pytest.mark.parametrize("lane", [0, 2])
def test_ordering_behind_a_submission(device, oracle, lane):
    """the oracle's picture uploaded into stream B, the packet submitted to stream A, the map asked for with nothing between: all zero, for I, P and B; then one
    byte of B changed: exactly that block"""
    st, dpb, nb = open_smoke_stream(device, lane)
    other = open_plain_stream(device, lane)
    try:
        view = D.frame_view(8, 6)
        gen = smoke_gop()
        for t, k in zip("IPB", (4, 3, 5)):
            pkt = gen.next_frame(t)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            oracle.decode_frame(pkt, dpb, 3)
            other.upload(0, dpb[d][:nb])
            st.submit(pkt)
            assert all_zero(st.blockdiff(d, view, other, 0, view, k)), t
            flipped = dpb[d][:nb].copy()
            at = view["offset"][1] + 21 * view["stride"][1] + 37
            flipped[at] ^= 0x80
            other.upload(0, flipped)
            got = st.blockdiff(d, view, other, 0, view, k)
            want = [np.zeros(m.shape, DT) for m in got]
            want[1][21 >> k, 37 >> k] = (128, 128 * 128)
            assert same(got, want), t
    finally:
        st.close()
        other.close()


@pytest.mark.parametrize("lane", [0, 2])
def test_ordering_behind_a_host_batch(device, oracle, lane):
    """submit_batch_host of three streams, then blockdiff_batch of the three against the oracle's pictures in three other streams, with nothing between"""
    sts = [open_smoke_stream(device, lane) for _ in range(3)]
    others = [open_plain_stream(device, lane) for _ in range(3)]
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
                    img[view["offset"][0] + 50 * view["stride"][0] + 100] ^= 1  # the second pair differs in one luma sample
                others[j].upload(0, img)
            device.submit_batch_host([s[0] for s in sts], pkts)
            got = device.blockdiff_batch([s[0] for s in sts], dst, [view] * 3, others, [0] * 3, [view] * 3, 4)
            assert all_zero(got[0]) and all_zero(got[2]), t
            want = [np.zeros(m.shape, DT) for m in got[1]]
            want[0][50 >> 4, 100 >> 4] = (1, 1)
            assert same(got[1], want), t
    finally:
        for s in sts:
            s[0].close()
        for s in others:
            s.close()


def test_errors(device):
    """every refusal is EINVAL with a text, leaves `out` untouched and queues nothing: a valid call right after it gives the right map"""
    lib = device.L
    rng = np.random.default_rng(9)
    a, b, other_lane, small = Slot(device, 5, 3, "pad16"), Slot(device, 5, 3, "tight"), Slot(device, 5, 3, "pad16", lane=1), Slot(device, 1, 1, "tight")
    large = Slot(device, 64, 32, "tight")  # 1024 x 512: a map of 98304 bytes at k = 3
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
        want = BD.frame_blockdiff(va, img_a, vb, img_b, 4)
        size = backend.blockdiff_bytes(va, 4)
        ca, cb = backend.as_view(va), backend.as_view(vb)
        out = np.full(2 * size + 64, 7, np.uint8)
        clone = backend.View.from_buffer_copy  # (as_view hands a View back as it is: a changed copy must not change the good one)

        def call(dev=device.h, streams_a=(a.st.h,), slots_a=(0,), views_a=(ca,), streams_b=(b.st.h,), slots_b=(0,), views_b=(cb,), n=None, k=4, res=out.ctypes.data, pitch=size):
            m = len(streams_a) if streams_a is not None else 1
            arr = lambda t, x: (t * len(x))(*x) if x is not None else None
            return lib.e264hip_blockdiff_batch(dev, arr(C.c_void_p, streams_a), arr(C.c_int, slots_a), arr(backend.View, views_a),
                                               arr(C.c_void_p, streams_b), arr(C.c_int, slots_b), arr(backend.View, views_b), m if n is None else n, k, res, pitch)

        def refused(what, **kw):
            assert call(**kw) == errno.EINVAL, what
            assert backend.last_error(), what
            assert (out == 7).all(), what
            assert same(a.st.blockdiff(0, va, b.st, 0, vb, 4), want), f"after the refusal of {what}"

        refused("a null device", dev=None)
        for name in ("streams_a", "slots_a", "views_a", "streams_b", "slots_b", "views_b"):
            refused("null " + name, **{name: None})
        refused("null out", res=None)
        refused("a null stream of A", streams_a=(None,))
        refused("a null stream of B", streams_b=(None,))
        refused("n < 0", n=-1)
        refused("n > 4096", n=4097)
        for k in (-1, 0, 2, 7):
            refused(f"k = {k}", k=k)
            assert "log2_block" in backend.last_error()
        for side in ("slots_a", "slots_b"):
            refused(side + ": slot -1", **{side: (-1,)})
            refused(side + ": slot past the table", **{side: (P.MAX_SLOTS,)})
            refused(side + ": a slot that is not allocated", **{side: (5,)})
        refused("streams of two lanes across the two sides", streams_b=(other_lane.st.h,), views_b=(ca,))
        two = dict(slots_a=(0, 0), views_a=(ca, ca), slots_b=(0, 0), pitch=size)
        refused("streams of two lanes on side A", streams_a=(a.st.h, other_lane.st.h), streams_b=(b.st.h, b.st.h), views_b=(cb, cb), **two)
        refused("streams of two lanes on side B", streams_a=(a.st.h, a.st.h), streams_b=(b.st.h, other_lane.st.h), views_b=(cb, ca), **two)
        refused("a stream of another device on side B", streams_b=(foreign.st.h,))
        refused("a stream of another device on side A", streams_a=(foreign.st.h,), views_a=(cb,))
        for side, good in (("views_a", ca), ("views_b", cb)):
            bad = clone(good)
            bad.plane[2].height += 4096
            refused(side + ": a view that leaves the slot", **{side: (bad,)})
            bad = clone(good)
            bad.plane[1].width = 0
            refused(side + ": a plane without samples", **{side: (bad,)})
            bad = clone(good)
            bad.plane[0].stride = bad.plane[0].width - 1
            refused(side + ": a stride below the width", **{side: (bad,)})
        bad = clone(cb)
        bad.plane[1].width = 0
        refused("the second pair's view", streams_a=(a.st.h, a.st.h), streams_b=(b.st.h, b.st.h), views_b=(cb, bad), **two)
        luma = clone(cb)
        luma.plane[0].width -= 2
        refused("luma widths differ", views_b=(luma,))
        chroma = clone(ca)
        chroma.plane[1].height -= 1
        chroma.plane[2].height -= 1
        refused("chroma heights differ", views_a=(chroma,))
        chroma = clone(cb)
        chroma.plane[2].width -= 1
        refused("Cr widths differ", views_b=(chroma,))
        whole_a = backend.as_view(D.frame_view(5, 3, geometry=b.geo))
        refused("a view valid for A's slot, not for B's smaller one", streams_a=(b.st.h,), views_a=(whole_a,), streams_b=(small.st.h,), views_b=(whole_a,))
        # pitch and cap
        refused("a pitch one byte short", pitch=size - 1)
        assert "pitch" in backend.last_error()
        refused("a pitch of 0", pitch=0)
        refused("the second pair's map larger than the pitch", streams_a=(small.st.h, a.st.h), slots_a=(0, 0), views_a=(backend.as_view(D.frame_view(1, 1, geometry=small.geo)), ca),
                streams_b=(small.st.h, b.st.h), slots_b=(0, 0), views_b=(backend.as_view(D.frame_view(1, 1, geometry=small.geo)), cb), pitch=size - 8)
        o = out.ctypes.data
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), b.st.h, 0, C.byref(cb), 4, o, size - 1) == errno.EINVAL and "cap" in backend.last_error()
        # more than E264_BLOCKDIFF_MAX_BYTES in one call: 4096 maps of 98304 bytes
        vl = backend.as_view(D.frame_view(64, 32, geometry=large.geo))
        big = backend.blockdiff_bytes(vl, 3)
        assert big == 98304 and 4096 * big > backend.BLOCKDIFF_MAX_BYTES >= 2730 * big
        refused("more than E264_BLOCKDIFF_MAX_BYTES", streams_a=(large.st.h,) * 4096, slots_a=(0,) * 4096, views_a=(vl,) * 4096, streams_b=(large.st.h,) * 4096,
                slots_b=(0,) * 4096, views_b=(vl,) * 4096, k=3, pitch=big)
        assert "E264_BLOCKDIFF_MAX_BYTES" in backend.last_error()
        # frame_blockdiff, the batch of one
        assert lib.e264hip_frame_blockdiff(None, 0, C.byref(ca), b.st.h, 0, C.byref(cb), 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), None, 0, C.byref(cb), 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, None, b.st.h, 0, C.byref(cb), 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), b.st.h, 0, None, 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), b.st.h, 0, C.byref(cb), 4, None, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 7, C.byref(ca), b.st.h, 0, C.byref(cb), 4, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), b.st.h, 0, C.byref(cb), 9, o, size) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), other_lane.st.h, 0, C.byref(ca), 4, o, size) == errno.EINVAL and backend.last_error()
        with pytest.raises(backend.BackendError):
            a.st.blockdiff(0, va, b.st, 0, luma, 4)
        with pytest.raises(ValueError):
            a.st.blockdiff(0, va, b.st, 0, vb, 2)
        with pytest.raises(ValueError):
            device.blockdiff_batch([a.st], [0], [va], [b.st], [0], [], 4)
        # n == 0 is no error, with or without arrays
        assert call(n=0) == 0 and call(streams_a=None, slots_a=None, views_a=None, streams_b=None, slots_b=None, views_b=None, n=0, res=None, pitch=0) == 0
        assert device.blockdiff_batch([], [], [], [], [], [], 4) == []
        assert (out == 7).all()  # no call above wrote anything
        # a cap larger than the map: only the map's bytes are written
        assert lib.e264hip_frame_blockdiff(a.st.h, 0, C.byref(ca), b.st.h, 0, C.byref(cb), 4, o, out.nbytes) == 0
        assert (out[:size].copy().view(DT) == np.concatenate([m.reshape(-1) for m in want])).all() and (out[size:] == 7).all()
        assert all_zero(other_lane.st.blockdiff(0, va, other_lane.st, 0, va, 4))  # (the stream of the other lane)
        assert all_zero(foreign.st.blockdiff(0, vb, foreign.st, 0, vb, 4))        # (... and of the other device object)
    finally:
        for s in (a, b, other_lane, small, large, foreign):
            s.close()
        dev2.close()


def md5s(frames):
    return [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames]


@pytest.mark.parametrize("download", [1, 0], ids=["download", "no-download"])
@pytest.mark.parametrize("name", ["crop_longterm_mmco", "mvc_ipp", "hd1080_ippb"])
def test_front_end(name, download):
    """e264front_frame_blockdiff over consecutive output frames fetched with borrow = 1 (the earlier one kept until the comparison, then returned), with read-back
    on and off, equals blockdiff_plane over the planes a second, downloading decoder delivered, which are the reference's; the block size goes round 3 .. 6"""
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
    ks = [KS[i % 4] for i in range(len(frames) - 1)]
    want = [[[BD.blockdiff_plane(p, q, k) for p, q in zip(cur[3 * v:3 * v + 3], prev[3 * v:3 * v + 3])] for v in range(n_views)] for prev, cur, k in zip(frames, frames[1:], ks)]
    assert any(BD.changed(m).any() for fr in want for v in fr for m in v)
    assert os.path.exists(FRONT_DIGEST), f"{FRONT_DIGEST} missing (built by __graft_entry__.build() on every machine)"
    dlib = C.CDLL(FRONT_DIGEST)  # e264front_frame_blockdiff: edge264_amd/frontend/front_blockdiff.c, in the library beside the front library
    fn = dlib.e264front_frame_blockdiff
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint16)]
    buf = np.frombuffer(data + b"\0" * 64, np.uint8).copy()
    base, end = buf.ctypes.data, buf.ctypes.data + len(data)
    got, kept = [], []
    cap = 8 * (3 * (-(-frames[0][0].shape[1] // 8)) * (-(-frames[0][0].shape[0] // 8)))  # more than any map of these frames
    lib.e264front_set_download(download)
    try:
        dec = C.c_void_p(lib.edge264_alloc(0, None, None, 0, None, None, None))
        assert dec
        out = Edge264Frame()

        def one(cur, prev, va, vb, k):
            raw = np.full(cap, 7, np.uint8)
            dims = (C.c_uint16 * 6)()
            r = fn(dec, C.byref(cur), va, dec, C.byref(prev), vb, k, raw.ctypes.data, cap, dims)
            if r:
                assert (raw == 7).all()
                return r
            d = [(int(dims[2 * p]), int(dims[2 * p + 1])) for p in range(3)]
            size = 8 * sum(bw * bh for bw, bh in d)
            assert (raw[size:] == 7).all()
            return BD.split_map(raw, d)

        def drain():
            n = 0
            while lib.edge264_get_frame(dec, C.byref(out), 1) == 0:  # borrowed: the frame stays ours until edge264_return_frame
                n += 1
                cur = Edge264Frame()
                C.memmove(C.byref(cur), C.byref(out), C.sizeof(Edge264Frame))
                assert bool(cur.samples_mvc[0]) == (n_views == 2)
                if kept:
                    k = ks[len(got)]
                    got.append([one(cur, kept[0], v, v, k) for v in range(n_views)])
                    if n_views == 1:
                        assert one(cur, kept[0], 1, 0, k) == errno.EINVAL  # no second view
                    lib.edge264_return_frame(dec, kept[0].return_arg)
                    kept.clear()
                else:  # the first frame against itself
                    assert all_zero(one(cur, cur, 0, 0, 4))
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
        for v in range(n_views):
            assert same(g[v], w[v]), f"frame {i + 1} against frame {i}, view {v}, k {ks[i]}"
    if name == "crop_longterm_mmco":
        assert frames[0][0].shape != (sums[name]["height_mbs"] * 16, sums[name]["width_mbs"] * 16), "the stream is cropped"


def yuv_frames(path, w, h):
    data = np.fromfile(path, np.uint8)
    fb = w * h * 3 // 2
    assert len(data) % fb == 0
    return [data[j:j + fb] for j in range(0, len(data), fb)]


def planes_of(f, w, h):
    return f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)


def parse_blockdiff_file(path):
    """the records of s<k>.blockdiff: [(k, [Y, Cb, Cr maps])]"""
    data, at, out = open(path, "rb").read(), 0, []
    while at < len(data):
        d = struct.unpack_from("<6HI", data, at)
        at += 16
        dims, k = [(d[0], d[1]), (d[2], d[3]), (d[4], d[5])], d[6]
        size = 8 * sum(bw * bh for bw, bh in dims)
        assert at + size <= len(data)
        out.append((k, BD.split_map(np.frombuffer(data, np.uint8, size, at), dims)))
        at += size
    return out


def test_driver_blockdiff_mode(tmp_path):
    """e264_multi --blockdiff DIR --out DIR2 on two committed streams: every record of s<k>.blockdiff is the map of consecutive frames of s<k>.yuv, whose frames
    are the reference's, at the default block size; --no-download --diff --blockdiff --blockdiff-log2 3 together writes the maps at 8 x 8 and the same .diff
    lines as --diff alone; refused with --parse-only and for a block size outside 3..6"""
    for p in (EXE, FRONT, HIP, FRONT_DIGEST):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["ipb_spatial", "tall_narrow"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out_dir, bd_dir, bd2_dir, diff_dir, diff2_dir = (tmp_path / d for d in ("out", "bd", "bd2", "diff", "diff2"))
    for d in (out_dir, bd_dir, bd2_dir, diff_dir, diff2_dir):
        d.mkdir()
    common = [EXE, "--front", FRONT, "--hip", HIP, "--threads", "2"]
    r1 = subprocess.run(common + ["--blockdiff", str(bd_dir), "--out", str(out_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(common + ["--no-download", "--diff", str(diff2_dir), "--blockdiff", str(bd2_dir), "--blockdiff-log2", "3"] + files, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    r3 = subprocess.run(common + ["--no-download", "--diff", str(diff_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r3.returncode == 0, r3.stderr[-2000:]
    s1, s2, s3 = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (r1, r2, r3))
    assert s1["frames"] == s2["frames"] == s3["frames"] == sum(len(sums[n]["md5"]) for n in names)
    changed = 0
    for i, n in enumerate(names):
        assert sums[n]["views"] == 1
        w, h = sums[n]["width_mbs"] * 16, sums[n]["height_mbs"] * 16
        frames = yuv_frames(out_dir / f"s{i}.yuv", w, h)
        assert [hashlib.md5(f.tobytes()).hexdigest() for f in frames] == sums[n]["md5"], f"stream {i} ({n})"
        for d, k in ((bd_dir, 4), (bd2_dir, 3)):
            recs = parse_blockdiff_file(d / f"s{i}.blockdiff")
            assert len(recs) == len(frames) - 1
            for j, (rk, maps) in enumerate(recs):
                want = [BD.blockdiff_plane(p, q, k) for p, q in zip(planes_of(frames[j + 1], w, h), planes_of(frames[j], w, h))]
                assert rk == k and same(maps, want), (n, j, k)
                changed += int(sum(BD.changed(m).sum() for m in maps))
        assert (diff2_dir / f"s{i}.diff").read_text() == (diff_dir / f"s{i}.diff").read_text() != "", f"stream {i} ({n}): --diff with and without --blockdiff"
    assert changed > 20
    r4 = subprocess.run(common + ["--parse-only", "--blockdiff", str(bd_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r4.returncode == 2 and "--blockdiff" in r4.stderr
    r5 = subprocess.run(common + ["--blockdiff", str(bd_dir), "--blockdiff-log2", "7"] + files, capture_output=True, text=True, timeout=600)
    assert r5.returncode == 2 and "--blockdiff-log2" in r5.stderr
