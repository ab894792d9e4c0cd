"""The block difference map (include/edge264_hip.h, version 1) without a GPU: its definition in numpy, in C and in a plain loop against known answers and each
other, the sum invariant against the difference record, the kernel's own body on the host under the address and undefined-behaviour sanitizers
(tests/emu/blockdiff_asan.cpp, a stand-alone program; both decompositions), the kernel's register budget from a cross-compilation, the library's and the front
library's entry points, and the refusals that need no device.  tests/test_hip_blockdiff.py runs the kernel.  Everything is compared for equality: there is no
tolerance anywhere."""
import ctypes as C
import errno
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from edge264_amd import backend, blockdiff as BD, diff as DF, digest as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SIZES = (1, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 129)
KS = (3, 4, 5, 6)


def plain_loop(a, b, k):
    """the definition, one sample at a time: [[(sad, sse)]] of bh rows of bw blocks"""
    h, w = len(a), len(a[0])
    bs = 1 << k
    bw, bh = (w + bs - 1) >> k, (h + bs - 1) >> k
    out = [[[0, 0] for _ in range(bw)] for _ in range(bh)]
    for y in range(h):
        for x in range(w):
            d = abs(a[y][x] - b[y][x])
            r = out[y >> k][x >> k]
            r[0] += d
            r[1] += d * d
    return [[tuple(r) for r in row] for row in out]


def as_lists(m):
    return [[(int(r["sad"]), int(r["sse"])) for r in row] for row in m]


class CBlockDiff(C.Structure):
    _fields_ = [("sad", C.c_uint32), ("sse", C.c_uint32)]


@pytest.fixture(scope="module")
def c_blockdiff(tmp_path_factory):
    """include/edge264_blockdiff.h in a temporary library: the header compiles as C++ with every warning an error, alone and behind edge264_hip.h"""
    if not shutil.which("g++"):
        pytest.fail("no g++")
    d = tmp_path_factory.mktemp("blockdiff_c")
    src = d / "blockdiff_c.cpp"
    src.write_text('#include "edge264_blockdiff.h"\n'
                   'extern "C" void bd_plane(const unsigned char *a, unsigned long sa, const unsigned char *b, unsigned long sb, unsigned w, unsigned h, int k, E264BlockDiff *out) '
                   '{ e264_blockdiff_plane(a, sa, b, sb, w, h, k, out); }\n'
                   'extern "C" int bd_dims(unsigned w, unsigned h, int k, unsigned *bw, unsigned *bh) { return e264_blockdiff_dims(w, h, k, bw, bh); }\n'
                   'extern "C" int bd_version(void) { return EDGE264_BLOCKDIFF_VERSION; }\n'
                   'extern "C" int bd_sizeof(void) { return (int)sizeof(E264BlockDiff); }\n')
    lib = d / "libblockdiff_c.so"
    flags = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include")]
    r = subprocess.run(flags + [str(src), "-o", str(lib)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    both = d / "both.cpp"
    both.write_text('#include "edge264_hip.h"\n#include "edge264_blockdiff.h"\n'
                    'static_assert(sizeof(E264BlockDiff) == 8 && E264_BLOCKDIFF_VERSION == EDGE264_BLOCKDIFF_VERSION && E264_BLOCKDIFF_MAX_BATCH == 4096 && '
                    'E264_BLOCKDIFF_MAX_BYTES == (1u << 28), "");\n'
                    'extern "C" int one(void) { return 1; }\n')
    r = subprocess.run(flags + [str(both), "-o", str(d / "libboth.so")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(lib))
    L.bd_plane.restype = None
    L.bd_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_void_p, C.c_ulong, C.c_uint, C.c_uint, C.c_int, C.POINTER(CBlockDiff)]
    L.bd_dims.argtypes = [C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    return L


def c_plane(L, a, b, k):
    """e264_blockdiff_plane of two 2-D arrays (rows any distance apart), with a guard record behind the map"""
    assert a.shape == b.shape and a.strides[1] == b.strides[1] == 1
    bw, bh = C.c_uint(), C.c_uint()
    assert L.bd_dims(a.shape[1], a.shape[0], k, C.byref(bw), C.byref(bh)) == 1
    n = bw.value * bh.value
    out = (CBlockDiff * (n + 1))()
    out[n].sad, out[n].sse = 0x5a5a5a5a, 0xa5a5a5a5
    L.bd_plane(a.ctypes.data, a.strides[0], b.ctypes.data, b.strides[0], a.shape[1], a.shape[0], k, out)
    assert (out[n].sad, out[n].sse) == (0x5a5a5a5a, 0xa5a5a5a5)
    return [[(out[y * bw.value + x].sad, out[y * bw.value + x].sse) for x in range(bw.value)] for y in range(bh.value)]


def all_three(L, a, b, k):
    got = BD.blockdiff_plane(a, b, k)
    bw, bh = BD.blockdiff_dims(a.shape[1], a.shape[0], k)
    assert got.shape == (bh, bw) and got.dtype == BD.BLOCKDIFF_DTYPE
    assert as_lists(got) == c_plane(L, a, b, k) == plain_loop(a.tolist(), b.tolist(), k), (a.shape, k)
    return got


def test_constants_and_dims(c_blockdiff):
    assert c_blockdiff.bd_version() == BD.BLOCKDIFF_VERSION == 1 and c_blockdiff.bd_sizeof() == 8 == BD.BLOCKDIFF_DTYPE.itemsize == backend.BLOCKDIFF_DTYPE.itemsize
    assert BD.BLOCKDIFF_DTYPE == backend.BLOCKDIFF_DTYPE and backend.BLOCKDIFF_MAX_BATCH == 4096 and backend.BLOCKDIFF_MAX_BYTES == 1 << 28
    bw, bh = C.c_uint(77), C.c_uint(77)
    for k in (-1, 0, 2, 7):
        assert c_blockdiff.bd_dims(16, 16, k, C.byref(bw), C.byref(bh)) == 0 and (bw.value, bh.value) == (77, 77)
        with pytest.raises(ValueError):
            BD.blockdiff_dims(16, 16, k)
    assert c_blockdiff.bd_dims(0, 16, 4, C.byref(bw), C.byref(bh)) == 0 and c_blockdiff.bd_dims(16, 0, 4, C.byref(bw), C.byref(bh)) == 0
    for k in KS:
        for w in SIZES:
            for h in (1, 64, 65):
                assert c_blockdiff.bd_dims(w, h, k, C.byref(bw), C.byref(bh)) == 1
                assert (bw.value, bh.value) == BD.blockdiff_dims(w, h, k) == (-(-w // (1 << k)), -(-h // (1 << k)))
    with pytest.raises(ValueError):
        BD.blockdiff_plane(np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.uint8), 3)
    with pytest.raises(ValueError):
        BD.blockdiff_plane(np.zeros((4, 4), np.uint16), np.zeros((4, 4), np.uint16), 3)


@pytest.mark.parametrize("k", KS)
def test_known_answers_numpy_c_and_plain_loop(c_blockdiff, k):
    """every w, h of SIZES: random planes in numpy, C and the plain loop; equal pictures; 0 against 255 everywhere; single changed samples at block corners"""
    rng = np.random.default_rng(160 + k)
    bs = 1 << k
    for w in SIZES:
        for h in SIZES:
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            b = rng.integers(0, 256, (h, w), dtype=np.uint8)
            bw, bh = BD.blockdiff_dims(w, h, k)
            if (w, h) in ((129, 129), (65, 33), (17, 9), (1, 1), (8, 64)) or w == h:
                got = all_three(c_blockdiff, a, b, k)  # (the plain loop is slow: a subset; the other sizes below in numpy and C)
            else:
                got = BD.blockdiff_plane(a, b, k)
                assert as_lists(got) == c_plane(c_blockdiff, a, b, k), (w, h)
            # the sum invariant against the difference record of the same planes
            whole = DF.diff_plane(a, b)
            assert int(got["sad"].sum(dtype=np.uint64)) == whole["sad"] and int(got["sse"].sum(dtype=np.uint64)) == whole["sse"]
            # equal pictures
            eq = BD.blockdiff_plane(a, a.copy(), k)
            assert not eq["sad"].any() and not eq["sse"].any() and not BD.changed(eq).any() and as_lists(eq) == c_plane(c_blockdiff, a, a.copy(), k)
            # 0 against 255: every record is its block's sample count times 255 and 255^2
            z, f = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
            ext = BD.blockdiff_plane(z, f, k)
            assert as_lists(ext) == c_plane(c_blockdiff, f, z, k)
            for Y in range(bh):
                for X in range(bw):
                    n = min(bs, h - bs * Y) * min(bs, w - bs * X)
                    assert (int(ext[Y, X]["sad"]), int(ext[Y, X]["sse"])) == (255 * n, 65025 * n)
            assert BD.changed(ext).all()
            # single changed samples at the corners of the last block (a partial one where w or h is no multiple of b) and of block (0, 0)
            for Y, X in ((0, 0), (bh - 1, bw - 1)):
                x0, y0, x1, y1 = bs * X, bs * Y, min(bs * X + bs, w) - 1, min(bs * Y + bs, h) - 1
                for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
                    c = a.copy()
                    c[y, x] ^= 0x83
                    d = abs(int(c[y, x]) - int(a[y, x]))
                    one = BD.blockdiff_plane(a, c, k)
                    want = np.zeros((bh, bw), BD.BLOCKDIFF_DTYPE)
                    want[Y, X] = (d, d * d)
                    assert (one == want).all() and as_lists(one) == c_plane(c_blockdiff, a, c, k), (w, h, x, y)
                    assert BD.changed(one).sum() == 1 and BD.changed(one)[Y, X]
    # the largest record: one 64 x 64 block of 0 against 255
    if k == 6:
        ext = all_three(c_blockdiff, np.zeros((64, 64), np.uint8), np.full((64, 64), 255, np.uint8), 6)
        assert as_lists(ext) == [[(4096 * 255, 4096 * 65025)]] and 4096 * 65025 < 1 << 32


def test_c_header_equals_numpy_on_strided_planes(c_blockdiff):
    """random planes, rows of the two sides at different distances, random bytes in the padding; frame_blockdiff over two slot images in different layouts"""
    rng = np.random.default_rng(264)
    for i in range(120):
        w, h, k = int(rng.integers(1, 140)), int(rng.integers(1, 140)), KS[i % 4]
        sa, sb = w + (0, 1, 3, 16)[i % 4], w + (0, 1, 3, 16)[(i // 4) % 4]
        A = rng.integers(0, 256, (h, sa), dtype=np.uint8)
        B = rng.integers(0, 256, (h, sb), dtype=np.uint8)
        if i % 3:  # B is A but for a few samples
            B[:, :w] = A[:, :w]
            for _ in range(i % 5):
                B[rng.integers(0, h), rng.integers(0, w)] ^= int(rng.integers(1, 256))
        assert c_plane(c_blockdiff, A[:, :w], B[:, :w], k) == as_lists(BD.blockdiff_plane(A[:, :w], B[:, :w], k)), (w, h, sa, sb, k)
    va, vb = D.frame_view(2, 1), D.frame_view(2, 1, geometry=dict(stride_Y=48, stride_C=48, plane_size_Y=48 * 16 + 7, plane_size_C=48 * 8))
    ia, ib = rng.integers(0, 256, 32 * 16 * 3 // 2, dtype=np.uint8), rng.integers(0, 256, 48 * 16 + 7 + 48 * 8, dtype=np.uint8)
    got = BD.frame_blockdiff(va, ia, vb, ib, 3)
    assert [m.shape for m in got] == [(2, 4), (1, 2), (1, 2)]
    whole = DF.frame_diff(va, ia, vb, ib)
    for m, r, p, q in zip(got, whole, D.view_planes(va, ia), D.view_planes(vb, ib)):
        assert (m == BD.blockdiff_plane(p, q, 3)).all() and int(m["sad"].sum()) == r["sad"] and int(m["sse"].sum()) == r["sse"]


def test_psnr_map_and_changed():
    a = np.zeros((20, 40), np.uint8)
    b = a.copy()
    b[0, 0] = 1        # block (0, 0) of 16 x 16: a mean squared error of 1 / 256
    b[19, 39] = 255    # block (1, 2) of 8 columns x 4 rows: 65025 / 32
    m = BD.blockdiff_plane(a, b, 4)
    ps = BD.psnr_map(m, 40, 20, 4)
    assert ps.shape == (2, 3) and ps[0, 0] == pytest.approx(10 * math.log10(65025.0 * 256), abs=1e-9) and ps[1, 2] == pytest.approx(10 * math.log10(32.0), abs=1e-9)
    assert np.isinf(ps[0, 1]) and np.isinf(ps[1, 0]) and np.isinf(ps).sum() == 4
    assert BD.changed(m).tolist() == [[True, False, False], [False, False, True]]
    with pytest.raises(ValueError):
        BD.psnr_map(m, 41, 20, 3)


@pytest.mark.parametrize("lane_groups", [0, 1], ids=["units-of-a-block", "lane-groups"])
def test_blockdiff_kernel_body_on_the_host_under_sanitizers(tmp_path, lane_groups):
    """tests/emu/blockdiff_asan.cpp: blockdiff_thread run over grids of 1 to 768 threads equals e264_blockdiff_plane for 6 widths x 3 heights x 4 x 4 strides x
    16 x 4 alignments x every k, every plane in a heap block of its own that ends with its last byte and the map in a block of exactly its size -- the sanitizers
    see no access outside the three -- every record stored exactly once, and 64 x 64 samples of 0 against 255 overflow nothing.  Both decompositions of
    e264_blockdiff.h: the shipped one and BD_LANE_GROUPS=1, whose cross-lane add the host wrapper emulates"""
    exe = str(tmp_path / "blockdiff_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        f"-DBD_LANE_GROUPS={lane_groups}", os.path.join(EMU, "blockdiff_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])
    m = re.search(r"blockdiff_asan: (\d+) cases, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == 6 * 3 * 4 * 4 * 16 * 4 * 4 + 8, r.stdout[-500:]


def test_blockdiff_kernel_resources(tmp_path):
    """e264_blockdiff.hip cross-compiled for gfx950: the kernel spills nothing, uses no scratch, no AGPRs, no LDS and at most the VGPRs its header states (BD_VGPRS)"""
    if not shutil.which(HIPCC):
        pytest.fail(f"no {HIPCC}: the cross-compiler is a tool of the build, not hardware")
    csrc = os.path.join(ROOT, "edge264_amd", "csrc")
    stated = re.search(r"^#define BD_VGPRS (\d+)", open(os.path.join(csrc, "e264_blockdiff.h")).read(), re.M)
    assert stated and 0 < int(stated.group(1)) <= 64, "the header states the VGPR count (eight waves per SIMD: at most 64)"
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(csrc, "e264_blockdiff.hip"), "-o", str(tmp_path / "b.o"),
                          "-Rpass-analysis=kernel-resource-usage", "-w"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(?:\S+:\s+)?([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    hits = {k: v for k, v in kernels.items() if "e264_blockdiff_kernel" in k}
    assert len(hits) == 1, sorted(kernels)
    r = next(iter(hits.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, r
    assert 0 < r["VGPRs"] <= int(stated.group(1)) and r["AGPRs"] == 0, r


def test_library_surface_and_host_only_refusals():
    """the library loads without a GPU and has the entry points; e264hip_blockdiff_bytes; e264hip_blockdiff_check -- what e264hip_blockdiff_batch runs for every
    pair before anything is queued -- refuses a block size outside 3..6, a bad view on either side and planes of different sizes, and names the cause; what the
    batch refuses before it looks at a device"""
    lib = backend.load_library()
    for name in ("e264hip_frame_blockdiff", "e264hip_blockdiff_batch", "e264hip_blockdiff_check", "e264hip_blockdiff_bytes"):
        assert hasattr(lib, name) and name in backend.EXPORTED_SYMBOLS
    # sizes
    v = D.frame_view(5, 3, crop=(2, 6, 2, 10))  # 72 x 36, chroma 36 x 18
    for k in KS:
        dims = [BD.blockdiff_dims(w, h, k) for w, h in zip(v["width"], v["height"])]
        assert backend.blockdiff_dims(v, k) == dims and backend.blockdiff_bytes(v, k) == 8 * sum(bw * bh for bw, bh in dims)
    assert backend.blockdiff_dims(v, 3) == [(9, 5), (5, 3), (5, 3)] and backend.blockdiff_dims(v, 6) == [(2, 1), (1, 1), (1, 1)]
    d = (C.c_uint16 * 6)(*[9] * 6)
    for k in (-1, 0, 2, 7, 64):
        assert lib.e264hip_blockdiff_bytes(C.byref(backend.as_view(v)), k, d) == 0 and list(d) == [9] * 6
        with pytest.raises(ValueError):
            backend.blockdiff_dims(v, k)
    assert backend.blockdiff_bytes(None, 4) == 0
    empty = backend.as_view(v)
    empty.plane[2].width = 0
    assert backend.blockdiff_bytes(empty, 4) == 0
    big = dict(offset=[0, 0, 0], stride=[65535] * 3, width=[65535] * 3, height=[65535] * 3)
    assert backend.blockdiff_bytes(big, 3) == 3 * 8192 * 8192 * 8 and backend.blockdiff_dims(big, 3) == [(8192, 8192)] * 3
    # the check: the diff's refusals and the range of k
    geo_a = dict(stride_Y=96, stride_C=104, plane_size_Y=96 * 48, plane_size_C=104 * 24)
    va, vb = D.frame_view(5, 3, crop=(2, 6, 2, 10), geometry=geo_a), D.frame_view(5, 3, crop=(4, 4, 0, 12))  # two layouts, two crops, one size
    na, nb = 96 * 48 + 104 * 24, 80 * 48 * 3 // 2
    for k in KS:
        assert backend.blockdiff_check(va, na, vb, nb, k) == 0 and backend.blockdiff_check(vb, nb, va, na, k) == 0 and backend.blockdiff_check(va, na, va, na, k) == 0
    for k in (-1, 0, 1, 2, 7, 8, 1 << 20):
        assert backend.blockdiff_check(va, na, vb, nb, k) == errno.EINVAL and "log2_block" in backend.last_error(), k
    assert lib.e264hip_blockdiff_check(None, na, C.byref(backend.as_view(vb)), nb, 4) == errno.EINVAL and "null" in backend.last_error()
    assert lib.e264hip_blockdiff_check(C.byref(backend.as_view(va)), na, None, nb, 4) == errno.EINVAL and "null" in backend.last_error()
    ea, eb = (max(o + (h - 1) * s + w for o, s, w, h in zip(x["offset"], x["stride"], x["width"], x["height"])) for x in (va, vb))  # the views' last bytes + 1
    assert eb < ea <= na and eb <= nb and backend.blockdiff_check(va, ea, vb, eb, 4) == 0
    assert backend.blockdiff_check(vb, eb - 1, vb, eb, 4) == errno.EINVAL and "leaves the slot" in backend.last_error()
    assert backend.blockdiff_check(vb, eb, vb, eb - 1, 4) == errno.EINVAL and "leaves the slot" in backend.last_error()
    assert backend.blockdiff_check(va, ea, va, eb, 4) == errno.EINVAL and "leaves the slot" in backend.last_error()  # valid for A's slot, not for B's smaller one
    for side in (0, 1):
        for p in range(3):
            for field, text in (("width", "without samples"), ("height", "without samples"), ("stride", "stride below width")):
                bad = backend.as_view(va)
                setattr(bad.plane[p], field, 0)
                pair = (bad, na, vb, nb) if side == 0 else (vb, nb, bad, na)
                assert backend.blockdiff_check(*pair, 5) == errno.EINVAL and text in backend.last_error(), (side, p, field)
    for p, name in enumerate(("Y", "Cb", "Cr")):
        for field in ("width", "height"):
            other = backend.as_view(vb)
            setattr(other.plane[p], field, getattr(other.plane[p], field) - 1)
            for pair in ((va, na, other, nb), (other, nb, va, na)):
                assert backend.blockdiff_check(*pair, 3) == errno.EINVAL, (p, field)
                assert "differ in size" in backend.last_error() and backend.last_error().endswith(name), backend.last_error()
    assert backend.blockdiff_check(va, na, vb, nb, 6) == 0
    # the batch, before it looks at a device: a null device, n < 0, n = 4097 -- EINVAL with a text, `out` untouched -- and n = 0 returns 0
    out = np.full(64, 7, np.uint8)
    for dev, n in ((None, 1), (None, -1), (None, 4097)):
        assert lib.e264hip_blockdiff_batch(dev, None, None, None, None, None, None, n, 4, out.ctypes.data, 64) == errno.EINVAL and backend.last_error()
    assert lib.e264hip_frame_blockdiff(None, 0, None, None, 0, None, 4, out.ctypes.data, 64) == errno.EINVAL and "null stream" in backend.last_error()
    assert (out == 7).all()


def test_front_blockdiff_library():
    """edge264_amd/libedge264_frontdigest.so exports e264front_frame_blockdiff (edge264_amd/frontend/front_blockdiff.c) beside the other passes' entry points,
    refuses null arguments, a view that is neither 0 nor 1 and a block size outside 3..6 before it looks for the front library or the back end, and answers
    ENODEV where the front library is not to be found"""
    path = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = C.CDLL(path)
    lib.e264front_frame_blockdiff.restype = C.c_int
    lib.e264front_frame_blockdiff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.e264front_frame_digest, lib.e264front_frame_preview, lib.e264front_frame_diff, lib.e264front_frame_hist, lib.e264front_digest_use  # (still there)
    out = np.full(256, 7, np.uint8)
    dims = (C.c_uint16 * 6)(*[9] * 6)
    frame = (C.c_char * 128)()
    o = out.ctypes.data
    assert lib.e264front_frame_blockdiff(None, frame, 0, 1, frame, 0, 4, o, 256, dims) == errno.EINVAL
    assert lib.e264front_frame_blockdiff(1, None, 0, 1, frame, 0, 4, o, 256, dims) == errno.EINVAL
    assert lib.e264front_frame_blockdiff(1, frame, 0, None, frame, 0, 4, o, 256, dims) == errno.EINVAL
    assert lib.e264front_frame_blockdiff(1, frame, 0, 1, None, 0, 4, o, 256, dims) == errno.EINVAL
    assert lib.e264front_frame_blockdiff(1, frame, 0, 1, frame, 0, 4, None, 256, dims) == errno.EINVAL
    for va, vb in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert lib.e264front_frame_blockdiff(1, frame, va, 1, frame, vb, 4, o, 256, dims) == errno.EINVAL
    for k in (-1, 0, 2, 7):
        assert lib.e264front_frame_blockdiff(1, frame, 0, 1, frame, 0, k, o, 256, dims) == errno.EINVAL
    assert (out == 7).all() and list(dims) == [9] * 6
    # without the front library: a copy of the library alone in a directory, in a process of its own (the binding is made once per process)
    code = ("import ctypes as C, shutil, sys, tempfile, os\n"
            "d = tempfile.mkdtemp()\n"
            "p = shutil.copy(sys.argv[1], os.path.join(d, 'libedge264_frontdigest.so'))\n"
            "os.environ.pop('E264_HIP_LIB', None)\n"
            "lib = C.CDLL(p)\n"
            "lib.e264front_frame_blockdiff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]\n"
            "f = (C.c_char * 128)(); o = (C.c_char * 96)()\n"
            "r = lib.e264front_frame_blockdiff(1, f, 0, 1, f, 0, 4, o, 96, None)\n"
            "shutil.rmtree(d)\n"
            "print(r)\n")
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and int(r.stdout.strip()) == errno.ENODEV, (r.stdout, r.stderr[-2000:])
