"""The digest kernel on the MI355X (e264hip_frame_digest / e264hip_digest_batch, include/edge264_hip.h): pictures verified where they lie in HBM.

Views: whole, cropped (Cb at an odd byte) and a 2 x 2 corner of pictures in the padded layouts of tests/layouts.py, against digest.plane_digest of the
host copy, and again with other random bytes everywhere outside the samples.  Sensitivity to single samples.  Ordering behind a submission, a fill
and a host batch with no wait between.  Batches of 1 to 257 pictures, mixed sizes and layouts.  Every refusal.  The front library on cropped, MVC
and 1080p streams with read-back off, and the driver's --digest mode.  tests/test_digest.py runs the kernel's body on the host first."""
import ctypes as C
import errno
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, digest as D, packet as P, synth
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
    """the three views of the issue: whole, cropped so that Cb starts at an odd byte, the bottom-right 2 x 2 luma / 1 x 1 chroma corner"""
    crop = (2, 2, 2, 2) if (w, h) == (1, 1) else (2, 6, 2, 10)
    return [D.frame_view(w, h, geometry=geo), D.frame_view(w, h, crop=crop, geometry=geo), D.frame_view(w, h, crop=(w * 16 - 2, 0, h * 16 - 2, 0), geometry=geo)]


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


PICTURES = [(w, h, lay) for (w, h) in ((1, 1), (5, 3), (17, 5), (130, 5)) for lay in ("tight", "pad16", "canvas", "gaps_wide")] + [(120, 68, "tight"), (128, 5, "tight")]


@pytest.mark.parametrize("w,h,layout", PICTURES, ids=[f"{w}x{h}-{lay}" for w, h, lay in PICTURES])
def test_views(device, w, h, layout):
    """whole, cropped and corner views: the device's digest is plane_digest of the host copy, and depends on the samples only"""
    rng = np.random.default_rng(w * 1000 + h)
    s = Slot(device, w, h, layout)
    try:
        if (w, layout) == (128, "tight"):
            assert s.geo["stride_Y"] == 2048 + 16  # the reference's layout never has a stride that is a multiple of 2048
        views = views_of(w, h, s.geo)
        assert views[1]["offset"][1] & 1, "Cb of the cropped view starts at an odd byte"
        assert all(backend.view_check(v, s.bytes) == 0 for v in views)
        img = L.random_slot(s.geo, rng)
        want = np.array([D.frame_digest(v, img) for v in views], np.uint64)
        s.upload(img)
        got = device.digest_batch([s.st] * 3, [0] * 3, views)
        assert got.shape == (3, 3) and got.dtype == np.uint64
        assert np.array_equal(got, want), (got, want)
        assert s.st.digest(0, views[1]) == tuple(int(x) for x in want[1])
        # the same samples, other random bytes in the padding, the gaps and the guard
        img2 = L.random_slot(s.geo, rng, samples_from=img)
        assert not np.array_equal(img, img2)
        s.upload(img2)
        assert np.array_equal(device.digest_batch([s.st] * 3, [0] * 3, views), want)
    finally:
        s.close()


def test_whole_picture_in_the_reference_layout_ends_the_slot(device):
    """Stream.digest's default view: a slot of exactly plane_size_Y + plane_size_C bytes, whose last byte is Cr's last sample"""
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (5, 3), (17, 5)):
        st = backend.Stream(device, w, h)
        try:
            st.alloc(0)
            img = rng.integers(0, 256, st.frame_bytes, dtype=np.uint8)
            st.upload(0, img)
            v = D.frame_view(w, h)
            assert v["offset"][2] + (v["height"][2] - 1) * v["stride"][2] + v["width"][2] == st.frame_bytes
            assert st.digest(0) == D.frame_digest(v, img)
        finally:
            st.close()


def test_sensitivity(device):
    """5 x 3 macroblocks, cropped view: one changed sample at either end of a plane's view changes that plane's value alone; a byte one column outside
    changes nothing"""
    rng = np.random.default_rng(11)
    s = Slot(device, 5, 3, "pad16")
    try:
        view = views_of(5, 3, s.geo)[1]
        img = L.random_slot(s.geo, rng)
        s.upload(img)
        base = s.st.digest(0, view)
        assert base == D.frame_digest(view, img)
        for p in range(3):
            o, sd, wd, ht = (view[k][p] for k in ("offset", "stride", "width", "height"))
            first, last = o, o + (ht - 1) * sd + wd - 1
            for at in (first, last):
                m = img.copy()
                m[at] ^= 1
                s.upload(m)
                got = s.st.digest(0, view)
                assert got[p] != base[p] and all(got[q] == base[q] for q in range(3) if q != p), (p, at, got, base)
                assert got == D.frame_digest(view, m)
            for at in (first - 1, last + 1):  # one column outside the view (samples of the picture the crop leaves out)
                m = img.copy()
                m[at] ^= 0xff
                s.upload(m)
                assert s.st.digest(0, view) == base, (p, at)
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
    """submit then digest with nothing between: the digest is the oracle's picture's, for I, P and B; then the same behind a fill"""
    st, dpb, nb = open_smoke_stream(device, lane)
    try:
        view = D.frame_view(8, 6)
        gen = smoke_gop()
        for t in "IPB":
            pkt = gen.next_frame(t)
            d = int(P.Packet(pkt).hdr["dst_slot"])
            st.submit(pkt)
            got = st.digest(d)
            oracle.decode_frame(pkt, dpb, 3)
            assert got == D.frame_digest(view, dpb[d][:nb]), t
        st.fill(3, 0x80)
        got = st.digest(3)
        assert got == (D.plane_digest(np.full((96, 128), 0x80, np.uint8)),) + (D.plane_digest(np.full((48, 64), 0x80, np.uint8)),) * 2
    finally:
        st.close()


def test_ordering_behind_a_host_batch(device, oracle):
    """submit_batch_host of three streams, then digest_batch of the three with nothing between"""
    sts = [open_smoke_stream(device) for _ in range(3)]
    try:
        gens = [smoke_gop(seed) for seed in (1, 2, 3)]
        view = D.frame_view(8, 6)
        for t in "IPB":
            pkts = [g.next_frame(t) for g in gens]
            dst = [int(P.Packet(p).hdr["dst_slot"]) for p in pkts]
            device.submit_batch_host([s[0] for s in sts], pkts)
            got = device.digest_batch([s[0] for s in sts], dst, [view] * 3)
            for k, (st, dpb, nb) in enumerate(sts):
                oracle.decode_frame(pkts[k], dpb, 3)
                assert tuple(int(x) for x in got[k]) == D.frame_digest(view, dpb[dst[k]][:nb]), (t, k)
    finally:
        for s in sts:
            s[0].close()


@pytest.fixture(scope="module")
def tiny_streams(device):
    """257 streams of 1 x 1-macroblock pictures with distinct contents, and what their digests must be"""
    rng = np.random.default_rng(257)
    geo = geo_of(1, 1, "tight")
    view = D.frame_view(1, 1, geometry=geo)
    slots, want = [], []
    for k in range(257):
        s = Slot(device, 1, 1, "tight")
        img = L.random_slot(geo, rng)
        s.upload(img)
        slots.append(s)
        want.append(D.frame_digest(view, img))
    assert len(set(want)) == 257
    yield slots, view, np.array(want, np.uint64)
    for s in slots:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_batches_of_small_pictures(device, tiny_streams, n):
    slots, view, want = tiny_streams
    got = device.digest_batch([s.st for s in slots[:n]], [0] * n, [view] * n)
    assert np.array_equal(got, want[:n])
    # results come in call order: the same streams the other way round
    got = device.digest_batch([s.st for s in reversed(slots[:n])], [0] * n, [view] * n)
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
            for v in views_of(s.w, s.h, s.geo)[:2]:
                streams.append(s.st); sl.append(0); views.append(v); want.append(D.frame_digest(v, img))
        other = L.random_slot(slots[1].geo, rng)  # the second slot of stream 1, in the same call as its first
        slots[1].upload(other, slot=1)
        v = views_of(5, 3, slots[1].geo)[0]
        streams.append(slots[1].st); sl.append(1); views.append(v); want.append(D.frame_digest(v, other))
        got = device.digest_batch(streams, sl, views)
        assert np.array_equal(got, np.array(want, np.uint64))
    finally:
        for s in slots:
            s.close()


def test_errors(device):
    """every refusal is EINVAL with a text and queues nothing: a valid call right after it gives the right digest"""
    lib = device.L
    rng = np.random.default_rng(9)
    a, b = Slot(device, 5, 3, "pad16"), Slot(device, 5, 3, "pad16", lane=1)
    try:
        img = L.random_slot(a.geo, rng)
        a.upload(img)
        b.upload(img)
        view = views_of(5, 3, a.geo)[1]
        want = D.frame_digest(view, img)
        cv = backend.as_view(view)
        out = (C.c_uint64 * 6)()

        def call(dev=device.h, streams=(a.st.h,), slots=(0,), views=(cv,), n=None, res=out):
            k = len(streams) if streams is not None else 1
            sa = (C.c_void_p * k)(*streams) if streams is not None else None
            la = (C.c_int * k)(*slots) if slots is not None else None
            va = (backend.View * k)(*views) if views is not None else None
            return lib.e264hip_digest_batch(dev, sa, la, va, k if n is None else n, res)

        def refused(what, **kw):
            assert call(**kw) == errno.EINVAL, what
            assert backend.last_error(), what
            assert a.st.digest(0, view) == want, f"after the refusal of {what}"

        refused("a null device", dev=None)
        refused("null streams", streams=None)
        refused("null slots", slots=None)
        refused("null views", views=None)
        refused("null out", res=None)
        refused("a null stream", streams=(None,))
        refused("n < 0", n=-1)
        refused("n > 4096", n=4097)
        refused("slot -1", slots=(-1,))
        refused("slot past the table", slots=(P.MAX_SLOTS,))
        refused("a slot that is not allocated", slots=(5,))
        bad = backend.as_view(view)
        bad.plane[2].height += 4096
        refused("a view that leaves the slot", views=(bad,))
        bad = backend.as_view(view)
        bad.plane[1].width = 0
        refused("a plane without samples", views=(bad,))
        refused("the second entry's view", streams=(a.st.h, a.st.h), slots=(0, 0), views=(cv, bad))
        refused("streams of two lanes", streams=(a.st.h, b.st.h), slots=(0, 0), views=(cv, cv))
        # frame_digest, the batch of one
        o3 = (C.c_uint64 * 3)()
        assert lib.e264hip_frame_digest(None, 0, C.byref(cv), o3) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_digest(a.st.h, 0, None, o3) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_digest(a.st.h, 0, C.byref(cv), None) == errno.EINVAL and backend.last_error()
        assert lib.e264hip_frame_digest(a.st.h, 7, C.byref(cv), o3) == errno.EINVAL and backend.last_error()
        # n == 0 is no error, with or without arrays
        assert call(n=0) == 0 and call(streams=None, slots=None, views=None, n=0, res=None) == 0
        assert device.digest_batch([], [], []).shape == (0, 3)
        assert b.st.digest(0, view) == want  # (the stream of the other lane)
    finally:
        a.close()
        b.close()


def md5s(frames):
    return [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames]


@pytest.mark.parametrize("name", ["crop_longterm_mmco", "mvc_ipp", "ipb_spatial", "hd1080_ippb"])
def test_front_end(name):
    """e264front_frame_digest with read-back off equals plane_digest of the planes a run with read-back on delivered, which are the reference's"""
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
    want = [[tuple(D.plane_digest(p) for p in fr[3 * v:3 * v + 3]) for v in range(len(fr) // 3)] for fr in frames]
    assert os.path.exists(FRONT_DIGEST), f"{FRONT_DIGEST} missing (built by __graft_entry__.build() on every machine)"
    dlib = C.CDLL(FRONT_DIGEST)  # e264front_frame_digest: edge264_amd/frontend/front_digest.c, a library beside the front library
    dlib.e264front_frame_digest.restype = C.c_int
    dlib.e264front_frame_digest.argtypes = [C.c_void_p, C.POINTER(Edge264Frame), C.c_int, C.POINTER(C.c_uint64)]
    buf = np.frombuffer(data + b"\0" * 64, np.uint8).copy()
    base, end = buf.ctypes.data, buf.ctypes.data + len(data)
    got = []
    lib.e264front_set_download(0)
    try:
        dec = C.c_void_p(lib.edge264_alloc(0, None, None, 0, None, None, None))
        assert dec
        out = Edge264Frame()
        d = (C.c_uint64 * 3)()

        def drain():
            while lib.edge264_get_frame(dec, C.byref(out), 0) == 0:
                views = []
                for v in range(2 if out.samples_mvc[0] else 1):
                    assert dlib.e264front_frame_digest(dec, C.byref(out), v, d) == 0
                    views.append(tuple(int(x) for x in d))
                if not out.samples_mvc[0]:
                    assert dlib.e264front_frame_digest(dec, C.byref(out), 1, d) == errno.EINVAL  # no second view
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
    assert got == want
    if name == "crop_longterm_mmco":
        assert frames[0][0].shape != (sums[name]["height_mbs"] * 16, sums[name]["width_mbs"] * 16), "the stream is cropped"
    if name == "mvc_ipp":
        assert all(len(v) == 2 for v in got)


def test_driver_digest_mode(tmp_path):
    """e264_multi --no-download --digest: every s<k>.digest holds the digests of that stream's frames from an --out run, whose frames are the reference's"""
    for p in (EXE, FRONT, HIP, FRONT_DIGEST):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["ipb_spatial", "t8x8_scaling", "slices_deblock_idc", "weighted_explicit", "one_mb", "tall_narrow", "i_4x4_16x16_pcm"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out_dir, dig_dir = tmp_path / "out", tmp_path / "digest"
    out_dir.mkdir()
    dig_dir.mkdir()
    common = [EXE, "--front", FRONT, "--hip", HIP, "--repeat", "3", "--threads", "3"]
    r1 = subprocess.run(common + ["--out", str(out_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(common + ["--no-download", "--digest", str(dig_dir)] + files, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    s1, s2 = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (r1, r2))
    assert s1["frames"] == s2["frames"] == 3 * sum(len(sums[n]["md5"]) for n in names)
    k = 0
    for _ in range(3):
        for n in names:
            assert sums[n]["views"] == 1
            w, h = sums[n]["width_mbs"] * 16, sums[n]["height_mbs"] * 16
            data = np.fromfile(out_dir / f"s{k}.yuv", np.uint8)
            fb = w * h * 3 // 2
            assert len(data) % fb == 0
            frames = [data[i:i + fb] for i in range(0, len(data), fb)]
            assert [hashlib.md5(f.tobytes()).hexdigest() for f in frames] == sums[n]["md5"], f"stream {k} ({n})"
            want = ["%016x %016x %016x" % (D.plane_digest(f[:w * h].reshape(h, w)), D.plane_digest(f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2)),
                                           D.plane_digest(f[w * h * 5 // 4:].reshape(h // 2, w // 2))) for f in frames]
            got = (dig_dir / f"s{k}.digest").read_text().splitlines()
            assert got == want, f"stream {k} ({n})"
            k += 1
