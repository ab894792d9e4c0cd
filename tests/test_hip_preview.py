"""The preview kernel on the MI355X (e264hip_frame_preview / e264hip_preview_batch, include/edge264_hip.h): pictures reduced by 2, 4 or 8 where they lie in HBM.

Views: whole, two crops (sizes that are no multiple of 8 with Cb at an odd byte; an odd chroma width) and a 2 x 2 corner of pictures in the padded layouts of
tests/layouts.py, against preview.frame_preview of the host copy, and again with other random bytes everywhere outside the samples.  A picture that ends its
slot.  `out` and `pitch`: not a byte outside the previews is written.  Ordering behind a submission, a fill and a host batch with no wait between.  Batches of
1 to 257 pictures, mixed sizes and layouts.  Every refusal.  The front library on cropped, MVC and 1080p streams with read-back off, and the driver's
--preview mode.  tests/test_preview.py runs the kernel's body on the host first."""
import ctypes as C
import errno
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, digest as D, packet as P, preview as PV, synth
from tests import layouts as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STREAMS = os.path.join(HERE, "golden", "streams")
EXE = os.path.join(ROOT, "edge264_amd", "e264_multi")
FRONT = os.path.join(ROOT, "edge264_amd", "libedge264_hipfront.so")
HIP = os.path.join(ROOT, "edge264_amd", "libedge264_hip.so")
FRONT_DIGEST = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
KS = (1, 2, 3)


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def geo_of(w, h, layout):
    return dict(width_mbs=w, height_mbs=h, **L.geometry(w, h, layout))


def views_of(w, h, geo):
    """the four views of the issue: whole; a crop to sizes that are no multiple of 8, Cb at an odd byte; a crop to an odd chroma width; the bottom-right
    2 x 2 luma / 1 x 1 chroma corner, where every box clamps"""
    return [D.frame_view(w, h, geometry=geo), D.frame_view(w, h, crop=(2, 6, 2, 10), geometry=geo), D.frame_view(w, h, crop=(6, 0, 2, 0), geometry=geo),
            D.frame_view(w, h, crop=(w * 16 - 2, 0, h * 16 - 2, 0), geometry=geo)]


def same(got, want):
    """two previews ([Y, Cb, Cr] arrays) are equal in shape, type and bytes"""
    return len(got) == len(want) == 3 and all(g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


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
    """whole, cropped and corner views at every reduction: the device's preview is frame_preview of the host copy, and depends on the samples only"""
    rng = np.random.default_rng(w * 1000 + h)
    s = Slot(device, w, h, layout)
    try:
        views = views_of(w, h, s.geo)
        assert views[1]["offset"][1] & 1, "Cb of the first cropped view starts at an odd byte"
        assert views[1]["width"][1] % 8 and views[1]["height"][0] % 8 and views[1]["height"][1] % 8 and views[2]["width"][1] & 1
        assert views[3]["width"] == [2, 1, 1] and views[3]["height"] == [2, 1, 1]
        assert all(backend.view_check(v, s.bytes) == 0 for v in views)
        img = L.random_slot(s.geo, rng)
        want = {k: [PV.frame_preview(v, img, k) for v in views] for k in KS}
        s.upload(img)
        for k in KS:
            got = device.preview_batch([s.st] * 4, [0] * 4, views, k)
            for i in range(4):
                assert same(got[i], want[k][i]), (k, i)
            assert same(s.st.preview(0, views[1], k), want[k][1]), k
        # the same samples, other random bytes in the padding, the gaps and the guard
        img2 = L.random_slot(s.geo, rng, samples_from=img)
        assert not np.array_equal(img, img2)
        s.upload(img2)
        for k in KS:
            got = device.preview_batch([s.st] * 4, [0] * 4, views, k)
            for i in range(4):
                assert same(got[i], want[k][i]), (k, i, "padding")
    finally:
        s.close()


def test_whole_picture_in_the_reference_layout_ends_the_slot(device):
    """Stream.preview's default view: a slot of exactly plane_size_Y + plane_size_C bytes, whose last byte is Cr's last sample"""
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (5, 3), (17, 5)):
        st = backend.Stream(device, w, h)
        try:
            st.alloc(0)
            img = rng.integers(0, 256, st.frame_bytes, dtype=np.uint8)
            st.upload(0, img)
            v = D.frame_view(w, h)
            assert v["offset"][2] + (v["height"][2] - 1) * v["stride"][2] + v["width"][2] == st.frame_bytes
            for k in KS:
                assert same(st.preview(0, k=k), PV.frame_preview(v, img, k)), (w, h, k)
            assert same(st.preview(0), PV.frame_preview(v, img, 3))  # k = 3 is the default
        finally:
            st.close()


def test_out_and_pitch(device):
    """pictures lie `pitch` apart in `out` and only their own bytes are written: with pitch = the preview's bytes + 37 in a buffer of 0xA5, every byte
    between the pictures and behind the last still is 0xA5; e264hip_frame_preview writes its preview and nothing behind it"""
    rng = np.random.default_rng(37)
    lib = device.L
    s = Slot(device, 5, 3, "pad16", n_slots=3)
    try:
        view = views_of(5, 3, s.geo)[1]
        imgs = [L.random_slot(s.geo, rng) for _ in range(3)]
        for i, img in enumerate(imgs):
            s.upload(img, slot=i)
        cv = backend.as_view(view)
        for k in KS:
            nb = backend.preview_bytes(view, k)
            assert nb == PV.preview_bytes(view, k)
            pitch = nb + 37
            out = np.full(3 * pitch + 11, 0xa5, np.uint8)
            sa, la, va = (C.c_void_p * 3)(*[s.st.h] * 3), (C.c_int * 3)(0, 1, 2), (backend.View * 3)(cv, cv, cv)
            assert lib.e264hip_preview_batch(device.h, sa, la, va, 3, k, out.ctypes.data, pitch) == 0, backend.last_error()
            for i, img in enumerate(imgs):
                want = np.concatenate([p.reshape(-1) for p in PV.frame_preview(view, img, k)])
                assert len(want) == nb and np.array_equal(out[i * pitch:i * pitch + nb], want), (k, i)
                assert (out[i * pitch + nb:(i + 1) * pitch] == 0xa5).all(), (k, i)
            assert (out[3 * pitch:] == 0xa5).all()
            one = np.full(nb + 37, 0xa5, np.uint8)
            assert lib.e264hip_frame_preview(s.st.h, 1, C.byref(cv), k, one.ctypes.data, nb) == 0, backend.last_error()
            assert np.array_equal(one[:nb], np.concatenate([p.reshape(-1) for p in PV.frame_preview(view, imgs[1], k)])) and (one[nb:] == 0xa5).all()
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
    """submit then preview with nothing between: the preview is the oracle's picture's, for I, P and B; then the same behind a fill"""
    st, dpb, nb = open_smoke_stream(device, lane)
    try:
        view = D.frame_view(8, 6)
        gen = smoke_gop()
        for i, t in enumerate("IPB"):
            k = KS[i]
            pkt = gen.next_frame(t)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            st.submit(pkt)
            got = st.preview(d, k=k)
            oracle.decode_frame(pkt, dpb, 3)
            assert same(got, PV.frame_preview(view, dpb[d][:nb], k)), t
        st.fill(3, 0x80)
        got = st.preview(3, k=2)
        assert same(got, [np.full((24, 32), 0x80, np.uint8), np.full((12, 16), 0x80, np.uint8), np.full((12, 16), 0x80, np.uint8)])
    finally:
        st.close()


def test_ordering_behind_a_host_batch(device, oracle):
    """submit_batch_host of three streams, then preview_batch of the three with nothing between"""
    sts = [open_smoke_stream(device) for _ in range(3)]
    try:
        gens = [smoke_gop(seed) for seed in (1, 2, 3)]
        view = D.frame_view(8, 6)
        for i, t in enumerate("IPB"):
            k = KS[2 - i]
            pkts = [g.next_frame(t) for g in gens]
            dst = [int(P.Packet(p).hdr["dst_slot"]) for p in pkts]
            device.submit_batch_host([s[0] for s in sts], pkts)
            got = device.preview_batch([s[0] for s in sts], dst, [view] * 3, k)
            for j, (st, dpb, nb) in enumerate(sts):
                oracle.decode_frame(pkts[j], dpb, 3)
                assert same(got[j], PV.frame_preview(view, dpb[dst[j]][:nb], k)), (t, j)
    finally:
        for s in sts:
            s[0].close()


@pytest.fixture(scope="module")
def tiny_streams(device):
    """257 streams of 1 x 1-macroblock pictures with distinct contents, and what their previews must be at k = 1"""
    rng = np.random.default_rng(257)
    geo = geo_of(1, 1, "tight")
    view = D.frame_view(1, 1, geometry=geo)
    slots, want = [], []
    for _ in range(257):
        s = Slot(device, 1, 1, "tight")
        img = L.random_slot(geo, rng)
        s.upload(img)
        slots.append(s)
        want.append(PV.frame_preview(view, img, 1))
    assert len({b"".join(p.tobytes() for p in w) for w in want}) == 257
    yield slots, view, want
    for s in slots:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_batches_of_small_pictures(device, tiny_streams, n):
    slots, view, want = tiny_streams
    got = device.preview_batch([s.st for s in slots[:n]], [0] * n, [view] * n, 1)
    assert len(got) == n and all(same(got[i], want[i]) for i in range(n))
    # results come in call order: the same streams the other way round
    got = device.preview_batch([s.st for s in reversed(slots[:n])], [0] * n, [view] * n, 1)
    assert len(got) == n and all(same(got[i], want[n - 1 - i]) for i in range(n))


def test_mixed_batch(device):
    """pictures of four sizes, each stream in its own layout (the seven of layouts.MIXED), whole and cropped views in one call; and one stream twice with two slots"""
    rng = np.random.default_rng(77)
    sizes = [(1, 1), (5, 3), (17, 5), (130, 5)]
    slots = [Slot(device, *sizes[i % 4], L.MIXED[i % len(L.MIXED)], n_slots=2 if i == 1 else 1) for i in range(8)]
    try:
        assert len({L.MIXED[i % len(L.MIXED)] for i in range(8)}) == 7
        streams, sl, views, imgs = [], [], [], []
        for s in slots:
            img = L.random_slot(s.geo, rng)
            s.upload(img)
            for v in views_of(s.w, s.h, s.geo)[:3]:
                streams.append(s.st); sl.append(0); views.append(v); imgs.append(img)
        other = L.random_slot(slots[1].geo, rng)  # the second slot of stream 1, in the same call as its first
        slots[1].upload(other, slot=1)
        streams.append(slots[1].st); sl.append(1); views.append(views_of(5, 3, slots[1].geo)[0]); imgs.append(other)
        for k in KS:
            got = device.preview_batch(streams, sl, views, k)
            assert len(got) == len(views)
            for i, (v, img) in enumerate(zip(views, imgs)):
                assert same(got[i], PV.frame_preview(v, img, k)), (k, i)
    finally:
        for s in slots:
            s.close()


def test_errors(device):
    """every refusal is EINVAL with a text and queues nothing: a valid call right after it gives the right picture"""
    lib = device.L
    rng = np.random.default_rng(9)
    a, b, big = Slot(device, 5, 3, "pad16"), Slot(device, 5, 3, "pad16", lane=1), Slot(device, 120, 68, "tight")
    try:
        img = L.random_slot(a.geo, rng)
        a.upload(img)
        b.upload(img)
        view = views_of(5, 3, a.geo)[1]
        want = PV.frame_preview(view, img, 2)
        nb = PV.preview_bytes(view, 2)
        cv = backend.as_view(view)
        out = np.zeros(2 * nb, np.uint8)

        def call(dev=device.h, streams=(a.st.h,), slots=(0,), views=(cv,), n=None, k=2, res=out.ctypes.data, pitch=nb):
            m = len(streams) if streams is not None else 1
            sa = (C.c_void_p * m)(*streams) if streams is not None else None
            la = (C.c_int * m)(*slots) if slots is not None else None
            va = (backend.View * m)(*views) if views is not None else None
            return lib.e264hip_preview_batch(dev, sa, la, va, m if n is None else n, k, res, pitch)

        def refused(what, **kw):
            assert call(**kw) == errno.EINVAL, what
            assert backend.last_error(), what
            assert same(a.st.preview(0, view, 2), want), f"after the refusal of {what}"

        refused("a null device", dev=None)
        refused("null streams", streams=None)
        refused("null slots", slots=None)
        refused("null views", views=None)
        refused("null out", res=None)
        refused("a null stream", streams=(None,))
        refused("n < 0", n=-1)
        refused("n > 4096", n=4097)
        for k in (0, 4, -1):
            refused(f"k = {k}", k=k)
        refused("slot -1", slots=(-1,))
        refused("slot past the table", slots=(P.MAX_SLOTS,))
        refused("a slot that is not allocated", slots=(5,))
        refused("streams of two lanes", streams=(a.st.h, b.st.h), slots=(0, 0), views=(cv, cv))
        bad = backend.as_view(view)
        bad.plane[2].height += 4096
        refused("a view that leaves the slot", views=(bad,))
        bad = backend.as_view(view)
        bad.plane[1].width = 0
        refused("a plane without samples", views=(bad,))
        refused("the second entry's view", streams=(a.st.h, a.st.h), slots=(0, 0), views=(cv, bad))
        refused("a pitch one byte short", pitch=nb - 1)
        refused("a pitch one byte short of the second picture", streams=(a.st.h, a.st.h), slots=(0, 0), views=(backend.as_view(views_of(5, 3, a.geo)[3]), cv), pitch=nb - 1)
        # more than E264_PREVIEW_MAX_BYTES in one call: 343 times the 1080p-sized picture at k = 1 (a stream may appear more than once); 342 would fit
        bv = D.frame_view(120, 68, geometry=big.geo)
        bb = PV.preview_bytes(bv, 1)
        assert bb % 16 == 0 and 343 * bb > backend.PREVIEW_MAX_BYTES >= 342 * bb and 343 <= backend.PREVIEW_MAX_BATCH
        room = np.empty(343 * bb, np.uint8)  # (never written: the call is refused)
        refused("more than E264_PREVIEW_MAX_BYTES", streams=(big.st.h,) * 343, slots=(0,) * 343, views=(backend.as_view(bv),) * 343, k=1, res=room.ctypes.data, pitch=bb)
        # frame_preview, the batch of one: cap is its pitch
        o = np.zeros(nb, np.uint8)
        assert lib.e264hip_frame_preview(None, 0, C.byref(cv), 2, o.ctypes.data, nb) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_preview(a.st.h, 0, None, 2, o.ctypes.data, nb) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_preview(a.st.h, 0, C.byref(cv), 2, None, nb) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_preview(a.st.h, 7, C.byref(cv), 2, o.ctypes.data, nb) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_preview(a.st.h, 0, C.byref(cv), 0, o.ctypes.data, nb) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_preview(a.st.h, 0, C.byref(cv), 2, o.ctypes.data, nb - 1) == errno.EINVAL and backend.last_error()
        assert not o.any()
        # n == 0 is no error, with or without arrays
        assert call(n=0) == 0 and call(streams=None, slots=None, views=None, n=0, res=None, pitch=0) == 0
        assert device.preview_batch([], [], []) == []
        assert not out.any()  # no call above wrote anything
        assert same(b.st.preview(0, view, 2), want)  # (the stream of the other lane)
    finally:
        a.close()
        b.close()
        big.close()


def md5s(frames):
    return [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames]


@pytest.mark.parametrize("name,k", [("crop_longterm_mmco", 3), ("crop_longterm_mmco", 1), ("mvc_ipp", 3), ("hd1080_ippb", 3)])
def test_front_end(name, k):
    """e264front_frame_preview with read-back off equals plane_preview of the planes a run with read-back on delivered, which are the reference's"""
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
    want = [[[PV.plane_preview(p, k) for p in fr[3 * v:3 * v + 3]] for v in range(len(fr) // 3)] for fr in frames]
    assert os.path.exists(FRONT_DIGEST), f"{FRONT_DIGEST} missing (built by __graft_entry__.build() on every machine)"
    dlib = C.CDLL(FRONT_DIGEST)  # e264front_frame_preview: edge264_amd/frontend/front_preview.c, in the library beside the front library
    dlib.e264front_frame_preview.restype = C.c_int
    dlib.e264front_frame_preview.argtypes = [C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint16)]
    buf = np.frombuffer(data + b"\0" * 64, np.uint8).copy()
    base, end = buf.ctypes.data, buf.ctypes.data + len(data)
    got = []
    cap = max(sum(p.size for p in v) for fr in want for v in fr)
    lib.e264front_set_download(0)
    try:
        dec = C.c_void_p(lib.edge264_alloc(0, None, None, 0, None, None, None))
        assert dec
        out = Edge264Frame()
        dims = (C.c_uint16 * 6)()

        def drain():
            while lib.edge264_get_frame(dec, C.byref(out), 0) == 0:
                views = []
                for v in range(2 if out.samples_mvc[0] else 1):
                    o = np.full(cap + 5, 0xa5, np.uint8)
                    assert dlib.e264front_frame_preview(dec, C.byref(out), v, k, o.ctypes.data, cap, dims) == 0
                    planes, at = [], 0
                    for p in range(3):
                        ow, oh = dims[2 * p], dims[2 * p + 1]
                        planes.append(o[at:at + ow * oh].reshape(oh, ow))
                        at += ow * oh
                    assert (o[at:] == 0xa5).all()
                    views.append(planes)
                    if len(got) == 0:
                        assert dlib.e264front_frame_preview(dec, C.byref(out), v, k, o.ctypes.data, at - 1, dims) == errno.EINVAL  # cap too small
                if not out.samples_mvc[0]:
                    assert dlib.e264front_frame_preview(dec, C.byref(out), 1, k, o.ctypes.data, cap, dims) == errno.EINVAL  # no second view
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
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(same(gv, wv) for gv, wv in zip(g, w)), f"frame {i}"
    if name == "crop_longterm_mmco":
        assert frames[0][0].shape != (sums[name]["height_mbs"] * 16, sums[name]["width_mbs"] * 16), "the stream is cropped"
    if name == "mvc_ipp":
        assert all(len(v) == 2 for v in got)


def test_driver_preview_mode(tmp_path):
    """e264_multi --no-download --preview (with --digest beside it): every s<k>.preview holds the previews of that stream's frames from an --out run, whose
    frames are the reference's"""
    for p in (EXE, FRONT, HIP, FRONT_DIGEST):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["ipb_spatial", "t8x8_scaling", "slices_deblock_idc", "weighted_explicit", "one_mb", "tall_narrow", "i_4x4_16x16_pcm"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out_dir, p3_dir, p1_dir, dig_dir = (tmp_path / d for d in ("out", "p3", "p1", "digest"))
    for d in (out_dir, p3_dir, p1_dir, dig_dir):
        d.mkdir()
    common = [EXE, "--front", FRONT, "--hip", HIP, "--repeat", "3", "--threads", "3"]
    r1 = subprocess.run(common + ["--out", str(out_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(common + ["--no-download", "--preview", str(p3_dir)] + files, capture_output=True, text=True, timeout=600)  # k = 3 is the default
    assert r2.returncode == 0, r2.stderr[-2000:]
    r3 = subprocess.run(common + ["--no-download", "--preview", str(p1_dir), "--preview-log2", "1", "--digest", str(dig_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r3.returncode == 0, r3.stderr[-2000:]
    s1, s2, s3 = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (r1, r2, r3))
    assert s1["frames"] == s2["frames"] == s3["frames"] == 3 * sum(len(sums[n]["md5"]) for n in names)
    r4 = subprocess.run(common + ["--preview", str(p1_dir), "--preview-log2", "4"] + files, capture_output=True, text=True, timeout=600)
    assert r4.returncode == 2 and "--preview-log2" in r4.stderr
    i = 0
    for _ in range(3):
        for n in names:
            assert sums[n]["views"] == 1
            w, h = sums[n]["width_mbs"] * 16, sums[n]["height_mbs"] * 16
            data = np.fromfile(out_dir / f"s{i}.yuv", np.uint8)
            fb = w * h * 3 // 2
            assert len(data) % fb == 0
            frames = [data[j:j + fb] for j in range(0, len(data), fb)]
            assert [hashlib.md5(f.tobytes()).hexdigest() for f in frames] == sums[n]["md5"], f"stream {i} ({n})"
            for k, d in ((3, p3_dir), (1, p1_dir)):
                want = b"".join(PV.plane_preview(pl, k).tobytes() for f in frames
                                for pl in (f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)))
                assert (d / f"s{i}.preview").read_bytes() == want, f"stream {i} ({n}), k = {k}"
            want = ["%016x %016x %016x" % (D.plane_digest(f[:w * h].reshape(h, w)), D.plane_digest(f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2)),
                                           D.plane_digest(f[w * h * 5 // 4:].reshape(h // 2, w // 2))) for f in frames]
            assert (dig_dir / f"s{i}.digest").read_text().splitlines() == want, f"stream {i} ({n})"
            i += 1
