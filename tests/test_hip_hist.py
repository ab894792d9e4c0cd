"""The histogram kernel on the MI355X (e264hip_frame_hist / e264hip_hist_batch, include/edge264_hip.h): the sample values of pictures counted where they lie
in HBM.

Views: whole, two crops (Cb at an odd byte; an odd chroma width) and a 2 x 2 corner of pictures of five sizes in the padded layouts of tests/layouts.py, against
hist.frame_hist of the host copy, and again with other random bytes everywhere outside the samples.  Content the scatter can get wrong: black, one value per
16-column unit, fifteen equal bytes and one different at each position, a ramp, a checkerboard of 0 and 255, noise.  Ordering behind a submission, a fill and a
host batch with no wait between.  Batches of 1 to 257 pictures, a mixed batch.  Every refusal.  The front library on cropped, MVC and 1080p streams with
read-back on and off, and the driver's --hist mode.  Everything is compared for equality.  tests/test_hist.py runs the kernel's body on the host first."""
import ctypes as C
import errno
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, digest as D, hist as H, packet as P, synth
from tests import layouts as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STREAMS = os.path.join(HERE, "golden", "streams")
EXE = os.path.join(ROOT, "edge264_amd", "e264_multi")
FRONT = os.path.join(ROOT, "edge264_amd", "libedge264_hipfront.so")
HIP = os.path.join(ROOT, "edge264_amd", "libedge264_hip.so")
FRONT_DIGEST = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def geo_of(w, h, layout):
    return dict(width_mbs=w, height_mbs=h, **L.geometry(w, h, layout))


def views_of(w, h, geo):
    """the four views of tests/test_hip_diff.py: whole; a crop with Cb at an odd byte; a crop to an odd chroma width; the bottom-right 2 x 2 luma /
    1 x 1 chroma corner"""
    return [D.frame_view(w, h, geometry=geo), D.frame_view(w, h, crop=(2, 6, 2, 10), geometry=geo), D.frame_view(w, h, crop=(6, 0, 2, 0), geometry=geo),
            D.frame_view(w, h, crop=(w * 16 - 2, 0, h * 16 - 2, 0), geometry=geo)]


def sizes_of(view):
    return [w * h for w, h in zip(view["width"], view["height"])]


def same(got, want, what=None):
    """a device record against hist.frame_hist's: shape, type, every bin; and each plane's bins sum to w * h"""
    assert got.shape == want.shape == (3, 256) and got.dtype == np.uint32, what
    if not np.array_equal(got, want):
        p, v = (int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError(f"{what}: bin[{p}][{v}] is {int(got[p][v])}, expected {int(want[p][v])} ({int((got != want).sum())} bins differ)")


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


PICTURES = [(w, h, lay) for (w, h) in ((1, 1), (5, 3), (17, 5), (130, 5)) for lay in ("tight", "pad16", "canvas", "gaps_wide")] + [(120, 68, "tight")]


@pytest.mark.parametrize("w,h,layout", PICTURES, ids=[f"{w}x{h}-{lay}" for w, h, lay in PICTURES])
def test_views(device, w, h, layout):
    """whole, cropped and corner views: the device's record is frame_hist of the host copy, singly and as a batch of four, each plane's bins sum to its
    samples, and the record depends on the samples only"""
    rng = np.random.default_rng(w * 1000 + h + len(layout))
    s = Slot(device, w, h, layout)
    try:
        views = views_of(w, h, s.geo)
        assert views[1]["offset"][1] & 1 and views[2]["width"][1] & 1 and views[3]["width"] == [2, 1, 1]
        assert all(backend.view_check(v, s.bytes) == 0 for v in views)
        img = L.random_slot(s.geo, rng)
        want = [H.frame_hist(v, img) for v in views]
        s.upload(img)
        got = device.hist_batch([s.st] * 4, [0] * 4, views)
        assert got.shape == (4, 3, 256) and got.dtype == np.uint32
        for i in range(4):
            same(got[i], want[i], f"view {i} of the batch")
            same(s.st.hist(0, views[i]), want[i], f"view {i} alone")
            assert got[i].sum(axis=1, dtype=np.uint64).tolist() == sizes_of(views[i]), i
        # the same samples, other random bytes in the padding, the gaps and the guard
        img2 = L.random_slot(s.geo, rng, samples_from=img)
        assert not np.array_equal(img, img2)
        s.upload(img2)
        got = device.hist_batch([s.st] * 4, [0] * 4, views)
        for i in range(4):
            same(got[i], want[i], f"view {i}, other padding")
    finally:
        s.close()


def put_planes(geo, img, y, cb, cr):
    """the three planes written into a slot image"""
    W, Hh = geo["width_mbs"] * 16, geo["height_mbs"] * 16
    sy, sc, psy = geo["stride_Y"], geo["stride_C"], geo["plane_size_Y"]
    img[:sy * Hh].reshape(Hh, sy)[:, :W] = y
    c = img[psy:psy + sc * (Hh // 2)].reshape(Hh // 2, sc)
    c[:, :W // 2] = cb
    c[:, sc // 2:sc // 2 + W // 2] = cr


def contents(w, h, rng):
    """(name, Y, Cb, Cr) of the contents a scatter can get wrong, for a picture of w x h macroblocks.  Units are 16-column groups of a row of the WHOLE
    picture: the whole view's interior units are exactly these"""
    W, Hh = w * 16, h * 16

    def plane(f, shift, salt):
        hh, ww = Hh >> shift, W >> shift
        return f(np.arange(ww)[None, :], np.arange(hh)[:, None], salt).astype(np.uint8) * np.ones((hh, ww), np.uint8)

    def three(f):
        return plane(f, 0, 0), plane(f, 1, 1), plane(f, 1, 2)

    out = [("black", np.full((Hh, W), 16, np.uint8), np.full((Hh // 2, W // 2), 128, np.uint8), np.full((Hh // 2, W // 2), 128, np.uint8))]
    unit = lambda x, y, salt: (37 * (x >> 4) + 101 * y + 7 * salt) & 255
    out.append(("one value per unit",) + three(unit))
    for pos in range(16):
        out.append((f"fifteen equal and one different at {pos}",) + three(lambda x, y, salt: np.where((x & 15) == pos, unit(x, y, salt) + 1 + (x >> 4), unit(x, y, salt)) & 255))
    out.append(("ramp",) + three(lambda x, y, salt: (x + y) & 255))
    out.append(("checkerboard of 0 and 255",) + three(lambda x, y, salt: ((x + y + salt) & 1) * 255))
    out.append(("noise",) + tuple(rng.integers(0, 256, (Hh >> s, W >> s), dtype=np.uint8) for s in (0, 1, 1)))
    return out


@pytest.mark.parametrize("w,h,layout", [(17, 5, "pad16"), (120, 68, "tight")], ids=["17x5", "120x68"])
def test_contents(device, w, h, layout):
    """content the scatter can get wrong, in one workgroup and across the workgroups of a 1080p-sized picture: black puts a whole plane into ONE bin
    (2 088 960 luma samples at 120 x 68), flat units and flat dwords take the short paths, a ramp and noise the general one"""
    rng = np.random.default_rng(w + h)
    s = Slot(device, w, h, layout)
    try:
        whole, crop = views_of(w, h, s.geo)[:2]
        img = L.random_slot(s.geo, rng)
        for name, y, cb, cr in contents(w, h, rng):
            put_planes(s.geo, img, y, cb, cr)
            s.upload(img)
            want = np.stack([H.hist_plane(p) for p in (y, cb, cr)])
            assert want.sum(axis=1).tolist() == [w * h * 256, w * h * 64, w * h * 64]
            same(s.st.hist(0, whole), want, name)
            same(s.st.hist(0, crop), H.frame_hist(crop, img), name + ", cropped")  # (the crop moves the units against the content's)
            if name == "black":
                assert want[0][16] == w * h * 256 and want[1][128] == want[2][128] == w * h * 64
                got = s.st.hist(0, D.frame_view(w, h, crop=(0, 0, 0, 8), geometry=s.geo))  # (120 x 68: the 1920 x 1080 picture, 2 073 600 luma samples)
                assert [int(got[0][16]), int(got[1][128]), int(got[2][128])] == [w * 16 * (h * 16 - 8), w * 8 * (h * 8 - 4), w * 8 * (h * 8 - 4)] and int(got.sum()) == w * 24 * (h * 16 - 8)
    finally:
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
    """submit then hist with nothing between: the record is the oracle's picture's, for I, P and B; then the same behind a fill"""
    st, dpb, nb = open_smoke_stream(device, lane)
    try:
        view = D.frame_view(8, 6)
        gen = smoke_gop()
        for t in "IPB":
            pkt = gen.next_frame(t)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            st.submit(pkt)
            got = st.hist(d)
            oracle.decode_frame(pkt, dpb, 3)
            same(got, H.frame_hist(view, dpb[d][:nb]), t)
        st.fill(3, 0x80)
        want = np.zeros((3, 256), np.uint32)
        want[:, 0x80] = [128 * 96, 64 * 48, 64 * 48]
        same(st.hist(3), want, "behind a fill")
    finally:
        st.close()


def test_ordering_behind_a_host_batch(device, oracle):
    """submit_batch_host of three streams, then hist_batch of the three with nothing between"""
    sts = [open_smoke_stream(device) for _ in range(3)]
    try:
        gens = [smoke_gop(seed) for seed in (1, 2, 3)]
        view = D.frame_view(8, 6)
        for t in "IPB":
            pkts = [g.next_frame(t) for g in gens]
            dst = [int(P.Packet(p).hdr["dst_slot"]) for p in pkts]
            device.submit_batch_host([s[0] for s in sts], pkts)
            got = device.hist_batch([s[0] for s in sts], dst, [view] * 3)
            for k, (st, dpb, nb) in enumerate(sts):
                oracle.decode_frame(pkts[k], dpb, 3)
                same(got[k], H.frame_hist(view, dpb[dst[k]][:nb]), (t, k))
    finally:
        for s in sts:
            s[0].close()


@pytest.fixture(scope="module")
def tiny_streams(device):
    """257 streams of 1 x 1-macroblock pictures with distinct contents, and what their records must be"""
    rng = np.random.default_rng(257)
    geo = geo_of(1, 1, "tight")
    view = D.frame_view(1, 1, geometry=geo)
    slots, want = [], []
    for k in range(257):
        s = Slot(device, 1, 1, "tight")
        img = L.random_slot(geo, rng)
        s.upload(img)
        slots.append(s)
        want.append(H.frame_hist(view, img))
    assert len({w.tobytes() for w in want}) == 257
    yield slots, view, np.stack(want)
    for s in slots:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_batches_of_small_pictures(device, tiny_streams, n):
    slots, view, want = tiny_streams
    got = device.hist_batch([s.st for s in slots[:n]], [0] * n, [view] * n)
    assert got.shape == (n, 3, 256) and np.array_equal(got, want[:n])
    # results come in call order: the same streams the other way round
    got = device.hist_batch([s.st for s in reversed(slots[:n])], [0] * n, [view] * n)
    assert np.array_equal(got, want[:n][::-1])


def test_mixed_batch(device):
    """pictures of four sizes, each stream in its own layout (layouts.MIXED), whole and cropped views in one call; and one stream twice with two slots"""
    rng = np.random.default_rng(77)
    sizes = [(1, 1), (5, 3), (17, 5), (130, 5)]
    slots = [Slot(device, *sizes[k % 4], L.MIXED[k % len(L.MIXED)], n_slots=2 if k == 1 else 1) for k in range(8)]
    try:
        streams, sl, views, want = [], [], [], []
        for k, s in enumerate(slots):
            img = L.random_slot(s.geo, rng)
            s.upload(img)
            for v in views_of(s.w, s.h, s.geo)[:3]:
                streams.append(s.st); sl.append(0); views.append(v); want.append(H.frame_hist(v, img))
        other = L.random_slot(slots[1].geo, rng)  # the second slot of stream 1, in the same call as its first
        slots[1].upload(other, slot=1)
        v = views_of(5, 3, slots[1].geo)[0]
        streams.append(slots[1].st); sl.append(1); views.append(v); want.append(H.frame_hist(v, other))
        got = device.hist_batch(streams, sl, views)
        assert got.shape == (25, 3, 256)
        for k in range(25):
            same(got[k], want[k], k)
    finally:
        for s in slots:
            s.close()


def test_errors(device):
    """every refusal is EINVAL with a text that names the cause, leaves `out` untouched and queues nothing: a valid call right after it gives the right record"""
    lib = device.L
    rng = np.random.default_rng(9)
    a, b = Slot(device, 5, 3, "pad16"), Slot(device, 5, 3, "pad16", lane=1)
    dev2 = backend.Device(0)  # a second device object: its streams are not `device`'s
    foreign = Slot(dev2, 5, 3, "pad16")
    try:
        img = L.random_slot(a.geo, rng)
        for s in (a, b, foreign):
            s.upload(img)
        view = views_of(5, 3, a.geo)[1]
        want = H.frame_hist(view, img)
        cv = backend.as_view(view)
        out = np.full((2, 3, 256), 7, np.uint32)

        def call(dev=device.h, streams=(a.st.h,), slots=(0,), views=(cv,), n=None, res=out.ctypes.data):
            k = len(streams) if streams is not None else 1
            sa = (C.c_void_p * k)(*streams) if streams is not None else None
            la = (C.c_int * k)(*slots) if slots is not None else None
            va = (backend.View * k)(*views) if views is not None else None
            return lib.e264hip_hist_batch(dev, sa, la, va, k if n is None else n, res)

        def refused(what, text, **kw):
            assert call(**kw) == errno.EINVAL, what
            assert text in backend.last_error(), (what, backend.last_error())
            assert (out == 7).all(), what
            same(a.st.hist(0, view), want, f"after the refusal of {what}")

        refused("a null device", "null device", dev=None)
        refused("null streams", "null argument", streams=None)
        refused("null slots", "null argument", slots=None)
        refused("null views", "null argument", views=None)
        refused("null out", "null argument", res=None)
        refused("a null stream", "batch entry", streams=(None,))
        refused("n < 0", "n outside", n=-1)
        refused("n > 4096", "n outside", n=4097)
        refused("slot -1", "slot out of range", slots=(-1,))
        refused("slot past the table", "slot out of range", slots=(P.MAX_SLOTS,))
        refused("a slot that is not allocated", "not allocated", slots=(5,))
        refused("streams of two lanes", "one compute lane", streams=(a.st.h, b.st.h), slots=(0, 0), views=(cv, cv))
        refused("a stream of another device", "batch entry", streams=(foreign.st.h,))
        refused("a stream of another device behind a good one", "batch entry", streams=(a.st.h, foreign.st.h), slots=(0, 0), views=(cv, cv))
        bad = backend.as_view(view)
        bad.plane[2].height += 4096
        refused("a view that leaves the slot", "leaves the slot", views=(bad,))
        bad = backend.as_view(view)
        bad.plane[0].stride = bad.plane[0].width - 1
        refused("a stride below the width", "stride below width", views=(bad,))
        bad = backend.as_view(view)
        bad.plane[1].width = 0
        refused("a plane without samples", "without samples", views=(bad,))
        refused("the second entry's view", "without samples", streams=(a.st.h, a.st.h), slots=(0, 0), views=(cv, bad))
        # frame_hist, the batch of one
        o = out.ctypes.data
        assert lib.e264hip_frame_hist(None, 0, C.byref(cv), o) == errno.EINVAL and "null stream" in backend.last_error()
        assert lib.e264hip_frame_hist(a.st.h, 0, None, o) == errno.EINVAL and "null argument" in backend.last_error()
        assert lib.e264hip_frame_hist(a.st.h, 0, C.byref(cv), None) == errno.EINVAL and "null argument" in backend.last_error()
        assert lib.e264hip_frame_hist(a.st.h, 7, C.byref(cv), o) == errno.EINVAL and "not allocated" in backend.last_error()
        assert lib.e264hip_frame_hist(a.st.h, 0, C.byref(bad), o) == errno.EINVAL and "without samples" in backend.last_error()
        with pytest.raises(backend.BackendError):
            a.st.hist(0, bad)
        with pytest.raises(ValueError):
            device.hist_batch([a.st], [0], [])
        # n == 0 is no error, with or without arrays
        assert call(n=0) == 0 and call(streams=None, slots=None, views=None, n=0, res=None) == 0
        assert device.hist_batch([], [], []).shape == (0, 3, 256)
        assert (out == 7).all()  # no call above wrote anything
        same(b.st.hist(0, view), want, "the stream of the other lane")
        same(foreign.st.hist(0, view), want, "the stream of the other device object")
    finally:
        for s in (a, b, foreign):
            s.close()
        dev2.close()


def md5s(frames):
    return [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames]


@pytest.mark.parametrize("download", [1, 0], ids=["download", "no-download"])
@pytest.mark.parametrize("name", ["crop_longterm_mmco", "mvc_ipp", "hd1080_ippb"])
def test_front_end(name, download):
    """e264front_frame_hist, with read-back on and off, equals hist_plane of the planes a downloading decoder delivered, which are the reference's"""
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
    want = [[np.stack([H.hist_plane(p) for p in fr[3 * v:3 * v + 3]]) for v in range(n_views)] for fr in frames]
    assert os.path.exists(FRONT_DIGEST), f"{FRONT_DIGEST} missing (built by __graft_entry__.build() on every machine)"
    dlib = C.CDLL(FRONT_DIGEST)  # e264front_frame_hist: edge264_amd/frontend/front_hist.c, in the library beside the front library
    dlib.e264front_frame_hist.restype = C.c_int
    dlib.e264front_frame_hist.argtypes = [C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_void_p]
    buf = np.frombuffer(data + b"\0" * 64, np.uint8).copy()
    base, end = buf.ctypes.data, buf.ctypes.data + len(data)
    got = []
    lib.e264front_set_download(download)
    try:
        dec = C.c_void_p(lib.edge264_alloc(0, None, None, 0, None, None, None))
        assert dec
        out = Edge264Frame()

        def drain():
            while lib.edge264_get_frame(dec, C.byref(out), 0) == 0:
                assert bool(out.samples_mvc[0]) == (n_views == 2)
                views = []
                for v in range(n_views):
                    rec = np.full((3, 256), 7, np.uint32)
                    assert dlib.e264front_frame_hist(dec, C.byref(out), v, rec.ctypes.data) == 0, backend.last_error()
                    views.append(rec)
                if n_views == 1:
                    rec = np.full((3, 256), 7, np.uint32)
                    assert dlib.e264front_frame_hist(dec, C.byref(out), 1, rec.ctypes.data) == errno.EINVAL  # no second view
                    assert (rec == 7).all()
                got.append(views)
        nal = lib.edge264_find_start_code(base, end, 0) + 3
        while True:
            nxt = lib.edge264_find_start_code(nal, end, 0) if nal < end else end
            res = lib.edge264_decode_NAL(dec, nal, nxt, None, None)
            n0 = len(got)
            drain()
            if res == errno.ENOBUFS:
                assert len(got) > n0
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
            same(g[v], w[v], f"frame {i}, view {v}")
    if name == "crop_longterm_mmco":
        assert frames[0][0].shape != (sums[name]["height_mbs"] * 16, sums[name]["width_mbs"] * 16), "the stream is cropped"


def test_driver_hist_mode(tmp_path):
    """e264_multi --hist DIR on two small streams: every 3072 bytes of s<k>.hist are the record, little-endian, of the next frame of s<k>.yuv from an --out run,
    whose frames are the reference's; a --no-download --digest --hist run writes the same bytes, and its digest lines are those of the frames; --parse-only
    refuses --hist"""
    for p in (EXE, FRONT, HIP, FRONT_DIGEST):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["ipb_spatial", "tall_narrow"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out_dir, hist_dir, hist2_dir, dig_dir = (tmp_path / d for d in ("out", "hist", "hist2", "digest"))
    for d in (out_dir, hist_dir, hist2_dir, dig_dir):
        d.mkdir()
    common = [EXE, "--front", FRONT, "--hip", HIP, "--threads", "2"]
    r1 = subprocess.run(common + ["--hist", str(hist_dir), "--out", str(out_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(common + ["--no-download", "--digest", str(dig_dir), "--hist", str(hist2_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    s1, s2 = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (r1, r2))
    assert s1["frames"] == s2["frames"] == sum(len(sums[n]["md5"]) for n in names)
    for k, n in enumerate(names):
        assert sums[n]["views"] == 1
        w, h = sums[n]["width_mbs"] * 16, sums[n]["height_mbs"] * 16
        data = np.fromfile(out_dir / f"s{k}.yuv", np.uint8)
        fb = w * h * 3 // 2
        assert len(data) % fb == 0
        frames = [data[i:i + fb] for i in range(0, len(data), fb)]
        assert [hashlib.md5(f.tobytes()).hexdigest() for f in frames] == sums[n]["md5"], f"stream {k} ({n})"
        planes = [(f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)) for f in frames]
        want = np.stack([np.stack([H.hist_plane(p) for p in pl]) for pl in planes])
        for d in (hist_dir, hist2_dir):
            raw = (d / f"s{k}.hist").read_bytes()
            assert len(raw) == 3072 * len(frames), f"stream {k} ({n}) in {d.name}"
            got = np.frombuffer(raw, "<u4").reshape(len(frames), 3, 256)
            assert np.array_equal(got, want), f"stream {k} ({n}) in {d.name}"
        assert len({w_.tobytes() for w_ in want}) > 1
        dig = (dig_dir / f"s{k}.digest").read_text().splitlines()
        assert dig == ["%016x %016x %016x" % tuple(D.plane_digest(p) for p in pl) for pl in planes], f"stream {k} ({n})"
    r3 = subprocess.run(common + ["--parse-only", "--hist", str(hist_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r3.returncode == 2 and "--hist" in r3.stderr
