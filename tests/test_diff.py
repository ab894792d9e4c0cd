"""The difference record (include/edge264_hip.h, version 1) without a GPU: its definition in numpy, in C and in a plain loop against known answers and each
other, the diff kernel's own body on the host under the address and undefined-behaviour sanitizers (tests/emu/diff_asan.cpp, a stand-alone program), the
kernel's register budget from a cross-compilation, the library's and the front library's entry points, and the refusals that need no device.
tests/test_hip_diff.py runs the kernel.  Everything is compared for equality: there is no tolerance anywhere."""
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

from edge264_amd import backend, diff as DF, digest as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NONE = 0xffffffff


def rec(sad=0, sse=0, count=0, first=NONE, max=0):
    return dict(sad=sad, sse=sse, count=count, first=first, max=max)


def plain_loop(a, b):
    """the definition, one sample at a time"""
    h, w = len(a), len(a[0])
    r = rec()
    for y in range(h):
        for x in range(w):
            d = abs(int(a[y][x]) - int(b[y][x]))
            if d:
                r["sad"] += d
                r["sse"] += d * d
                r["count"] += 1
                r["max"] = max(r["max"], d)
                r["first"] = min(r["first"], y * w + x)
    return r


class CPlaneDiff(C.Structure):
    _fields_ = [("sad", C.c_uint64), ("sse", C.c_uint64), ("count", C.c_uint32), ("first", C.c_uint32), ("max", C.c_uint32), ("zero", C.c_uint32)]


@pytest.fixture(scope="module")
def c_diff(tmp_path_factory):
    """include/edge264_diff.h in a temporary library: the header compiles as C++ with every warning an error, alone and behind edge264_hip.h"""
    if not shutil.which("g++"):
        pytest.fail("no g++")
    d = tmp_path_factory.mktemp("diff_c")
    src = d / "diff_c.cpp"
    src.write_text('#include "edge264_diff.h"\n'
                   'extern "C" void diff_plane(const unsigned char *a, unsigned long sa, const unsigned char *b, unsigned long sb, unsigned w, unsigned h, E264PlaneDiff *out) '
                   '{ e264_diff_plane(a, sa, b, sb, w, h, out); }\n'
                   'extern "C" int diff_version(void) { return EDGE264_DIFF_VERSION; }\n'
                   'extern "C" int diff_sizeof(void) { return (int)sizeof(E264PlaneDiff); }\n')
    lib = d / "libdiff_c.so"
    flags = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include")]
    r = subprocess.run(flags + [str(src), "-o", str(lib)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    both = d / "both.cpp"
    both.write_text('#include "edge264_hip.h"\n#include "edge264_diff.h"\n'
                    'static_assert(sizeof(E264PlaneDiff) == 32 && sizeof(E264Diff) == 96 && E264_DIFF_VERSION == EDGE264_DIFF_VERSION && E264_DIFF_MAX_BATCH == 4096, "");\n'
                    'extern "C" unsigned none(void) { return E264_DIFF_NONE; }\n')
    r = subprocess.run(flags + [str(both), "-o", str(d / "libboth.so")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(lib))
    L.diff_plane.restype = None
    L.diff_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_void_p, C.c_ulong, C.c_uint, C.c_uint, C.POINTER(CPlaneDiff)]
    return L


def c_plane(L, a, b):
    """e264_diff_plane of two 2-D arrays (rows any distance apart)"""
    assert a.shape == b.shape and a.strides[1] == b.strides[1] == 1
    out = CPlaneDiff(1, 2, 3, 4, 5, 6)
    L.diff_plane(a.ctypes.data, a.strides[0], b.ctypes.data, b.strides[0], a.shape[1], a.shape[0], C.byref(out))
    assert out.zero == 0
    return rec(out.sad, out.sse, out.count, out.first, out.max)


def all_three(L, a, b):
    got = DF.diff_plane(a, b)
    assert got == c_plane(L, a, b) == plain_loop(a.tolist(), b.tolist())
    return got


def test_known_answers_numpy_c_and_plain_loop(c_diff):
    assert c_diff.diff_version() == DF.DIFF_VERSION == 1 and c_diff.diff_sizeof() == 32 == backend.DIFF_DTYPE.itemsize
    assert DF.DIFF_NONE == backend.DIFF_NONE == NONE
    rng = np.random.default_rng(14)
    w, h = 21, 6
    a = rng.integers(1, 255, (h, w), dtype=np.uint8)  # (1..254: every sample can move by 1 either way)
    # equal planes
    assert all_three(c_diff, a, a.copy()) == rec()
    z = np.zeros((h, w), np.uint8)
    assert all_three(c_diff, z, z.copy()) == rec()
    # one sample changed by 1: at index 0, at w * h - 1, at the last column of one row and the first of the next
    for i in (0, w * h - 1, 3 * w - 1, 3 * w):
        for step in (1, -1):
            b = a.copy()
            b.reshape(-1)[i] = int(b.reshape(-1)[i]) + step
            assert all_three(c_diff, a, b) == rec(1, 1, 1, i, 1) == all_three(c_diff, b, a), (i, step)
        # ... and by 255
        b = z.copy()
        b.reshape(-1)[i] = 255
        assert all_three(c_diff, z, b) == rec(255, 65025, 1, i, 255) == all_three(c_diff, b, z), i
    # two changed samples: first is the smaller index whatever their order of change
    for i, j in ((5, 100), (100, 5), (w - 1, w), (w, w - 1)):
        b = a.copy()
        b.reshape(-1)[i] += 3
        b.reshape(-1)[j] -= 1
        assert all_three(c_diff, a, b) == rec(4, 10, 2, min(i, j), 3), (i, j)
    # 0 against 255 everywhere
    f = np.full((h, w), 255, np.uint8)
    assert all_three(c_diff, z, f) == rec(255 * w * h, 65025 * w * h, w * h, 0, 255) == all_three(c_diff, f, z)
    # what has no record
    with pytest.raises(ValueError):
        DF.diff_plane(a, a[:, :-1])
    with pytest.raises(ValueError):
        DF.diff_plane(a.astype(np.uint16), a.astype(np.uint16))
    # psnr
    assert DF.psnr(0, 16, 16) == math.inf
    assert DF.psnr(256, 16, 16) == pytest.approx(10 * math.log10(65025.0), abs=1e-12)  # a mean squared error of 1


def test_c_header_equals_numpy(c_diff):
    """random planes, rows of the two sides at different distances, random bytes in the padding"""
    rng = np.random.default_rng(264)
    for i in range(200):
        w, h = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        sa, sb = w + (0, 1, 3, 16)[i % 4], w + (0, 1, 3, 16)[(i // 4) % 4]
        A = rng.integers(0, 256, (h, sa), dtype=np.uint8)
        B = rng.integers(0, 256, (h, sb), dtype=np.uint8)
        if i % 3:  # B is A but for a few samples
            B[:, :w] = A[:, :w]
            for _ in range(i % 5):
                B[rng.integers(0, h), rng.integers(0, w)] ^= int(rng.integers(1, 256))
        assert c_plane(c_diff, A[:, :w], B[:, :w]) == DF.diff_plane(A[:, :w], B[:, :w]), (w, h, sa, sb)
    # frame_diff over two slot images in different layouts
    va, vb = D.frame_view(2, 1), D.frame_view(2, 1, geometry=dict(stride_Y=48, stride_C=48, plane_size_Y=48 * 16 + 7, plane_size_C=48 * 8))
    ia, ib = rng.integers(0, 256, 32 * 16 * 3 // 2, dtype=np.uint8), rng.integers(0, 256, 48 * 16 + 7 + 48 * 8, dtype=np.uint8)
    got = DF.frame_diff(va, ia, vb, ib)
    assert len(got) == 3 and got == [DF.diff_plane(p, q) for p, q in zip(D.view_planes(va, ia), D.view_planes(vb, ib))] and got[0]["count"] > 400


def test_diff_kernel_body_on_the_host_under_sanitizers(tmp_path):
    """tests/emu/diff_asan.cpp: diff_thread run over grids of 1 to 768 threads, the partial records combined, equals e264_diff_plane for 6 widths x 2 heights x
    4 x 4 strides x 16 x 4 alignments x 4 kinds of change x 2 grids, every plane in a heap block of its own that ends with its last byte -- the sanitizers see no
    access outside either block -- and ONE thread over 4096 x 4096 samples of 0 against 255 overflows nothing"""
    exe = str(tmp_path / "diff_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "diff_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])
    m = re.search(r"diff_asan: (\d+) cases, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == 6 * 2 * 4 * 4 * 16 * 4 * 4 * 2 + 1, r.stdout[-500:]


def test_diff_kernel_resources(tmp_path):
    """e264_diff.hip cross-compiled for gfx950: the diff kernel spills nothing, uses no scratch and at most 128 VGPRs (four waves per SIMD stay resident)"""
    if not shutil.which(HIPCC):
        pytest.fail(f"no {HIPCC}: the cross-compiler is a tool of the build, not hardware")
    src = os.path.join(ROOT, "edge264_amd", "csrc", "e264_diff.hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "d.o"),
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
    hits = {k: v for k, v in kernels.items() if "e264_diff_kernel" in k}
    assert len(hits) == 1, sorted(kernels)
    r = next(iter(hits.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, r
    assert 0 < r["VGPRs"] <= 128 and r["AGPRs"] == 0, r


def test_library_surface_and_host_only_refusals():
    """the library loads without a GPU and has the entry points; e264hip_diff_check -- what e264hip_diff_batch runs for every pair before anything is queued --
    refuses a bad view on either side and planes of different sizes, and names the cause"""
    lib = backend.load_library()
    for name in ("e264hip_frame_diff", "e264hip_diff_batch", "e264hip_diff_check"):
        assert hasattr(lib, name) and name in backend.EXPORTED_SYMBOLS
    assert backend.DIFF_MAX_BATCH == 4096
    geo_a = dict(stride_Y=96, stride_C=104, plane_size_Y=96 * 48, plane_size_C=104 * 24)
    va, vb = D.frame_view(5, 3, crop=(2, 6, 2, 10), geometry=geo_a), D.frame_view(5, 3, crop=(4, 4, 0, 12))  # two layouts, two crops, one size
    na, nb = 96 * 48 + 104 * 24, 80 * 48 * 3 // 2
    assert va["width"] == vb["width"] and va["height"] == vb["height"] and va["offset"] != vb["offset"]
    assert backend.diff_check(va, na, vb, nb) == 0 and backend.diff_check(vb, nb, va, na) == 0 and backend.diff_check(va, na, va, na) == 0
    assert lib.e264hip_diff_check(None, na, C.byref(backend.as_view(vb)), nb) == errno.EINVAL and "null" in backend.last_error()
    assert lib.e264hip_diff_check(C.byref(backend.as_view(va)), na, None, nb) == errno.EINVAL and "null" in backend.last_error()
    # a view its own slot does not hold: A's in a slot one byte short, B's in a slot one byte short, each fine in the other's (larger) slot
    ea, eb = (max(o + (h - 1) * s + w for o, s, w, h in zip(v["offset"], v["stride"], v["width"], v["height"])) for v in (va, vb))  # the views' last bytes + 1
    assert eb < ea <= na and eb <= nb and backend.diff_check(va, ea, vb, eb) == 0
    assert backend.diff_check(vb, eb - 1, vb, eb) == errno.EINVAL and "leaves the slot" in backend.last_error()
    assert backend.diff_check(vb, eb, vb, eb - 1) == errno.EINVAL and "leaves the slot" in backend.last_error()
    assert backend.diff_check(va, ea, va, eb) == errno.EINVAL and "leaves the slot" in backend.last_error()  # valid for A's slot, not for B's smaller one
    for side in (0, 1):
        for p in range(3):
            for field, text in (("width", "without samples"), ("height", "without samples"), ("stride", "stride below width")):
                bad = backend.as_view(va)
                setattr(bad.plane[p], field, 0)
                pair = (bad, na, vb, nb) if side == 0 else (vb, nb, bad, na)
                assert backend.diff_check(*pair) == errno.EINVAL and text in backend.last_error(), (side, p, field)
    # planes of different sizes: luma only, chroma only, one plane's width, one plane's height
    for p, name in enumerate(("Y", "Cb", "Cr")):
        for field in ("width", "height"):
            other = backend.as_view(vb)
            setattr(other.plane[p], field, getattr(other.plane[p], field) - 1)
            for pair in ((va, na, other, nb), (other, nb, va, na)):
                assert backend.diff_check(*pair) == errno.EINVAL, (p, field)
                assert "differ in size" in backend.last_error() and backend.last_error().endswith(name), backend.last_error()
    luma = D.frame_view(5, 3, crop=(4, 4, 0, 12))
    luma["width"][0] -= 2
    assert backend.diff_check(va, na, luma, nb) == errno.EINVAL and backend.last_error().endswith(": Y")
    chroma = D.frame_view(5, 3, crop=(4, 4, 0, 12))
    chroma["height"][1] -= 1
    chroma["height"][2] -= 1
    assert backend.diff_check(va, na, chroma, nb) == errno.EINVAL and backend.last_error().endswith(": Cb")
    assert backend.diff_check(va, na, vb, nb) == 0


def test_front_diff_library():
    """edge264_amd/libedge264_frontdigest.so exports e264front_frame_diff (edge264_amd/frontend/front_diff.c) beside the digest's and the preview's entry points,
    refuses null arguments and a view that is neither 0 nor 1 before it looks for the front library or the back end, and answers ENODEV where the front
    library is not to be found"""
    path = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = C.CDLL(path)
    lib.e264front_frame_diff.restype = C.c_int
    lib.e264front_frame_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.e264front_frame_digest, lib.e264front_frame_preview, lib.e264front_digest_use  # (still there)
    out = np.full(3, 7, backend.DIFF_DTYPE)
    frame = (C.c_char * 128)()
    o = out.ctypes.data
    assert lib.e264front_frame_diff(None, frame, 0, 1, frame, 0, o) == errno.EINVAL
    assert lib.e264front_frame_diff(1, None, 0, 1, frame, 0, o) == errno.EINVAL
    assert lib.e264front_frame_diff(1, frame, 0, None, frame, 0, o) == errno.EINVAL
    assert lib.e264front_frame_diff(1, frame, 0, 1, None, 0, o) == errno.EINVAL
    assert lib.e264front_frame_diff(1, frame, 0, 1, frame, 0, None) == errno.EINVAL
    for va, vb in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert lib.e264front_frame_diff(1, frame, va, 1, frame, vb, o) == errno.EINVAL
    assert (out == np.full(3, 7, backend.DIFF_DTYPE)).all()
    # without the front library: a copy of the library alone in a directory, in a process of its own (the binding is made once per process)
    code = ("import ctypes as C, shutil, sys, tempfile, os\n"
            "d = tempfile.mkdtemp()\n"
            "p = shutil.copy(sys.argv[1], os.path.join(d, 'libedge264_frontdigest.so'))\n"
            "os.environ.pop('E264_HIP_LIB', None)\n"
            "lib = C.CDLL(p)\n"
            "lib.e264front_frame_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]\n"
            "f = (C.c_char * 128)(); o = (C.c_char * 96)()\n"
            "r = lib.e264front_frame_diff(1, f, 0, 1, f, 0, o)\n"
            "shutil.rmtree(d)\n"
            "print(r)\n")
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and int(r.stdout.strip()) == errno.ENODEV, (r.stdout, r.stderr[-2000:])
