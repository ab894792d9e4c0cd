"""The histogram record (include/edge264_hip.h, version 1) without a GPU: its definition in numpy, in C and in a plain loop against known answers and each
other, the arithmetic on the bins (stats, quantile, distance) against numpy's own, the histogram kernel's own body on the host under the address and
undefined-behaviour sanitizers (tests/emu/hist_asan.cpp, a stand-alone program), the kernel's register budget from a cross-compilation, the library's and the
front library's entry points, and the refusals that need no device.  tests/test_hip_hist.py runs the kernel.  Everything is compared for equality: there is no
tolerance anywhere."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from edge264_amd import backend, digest as D, hist as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def plain_loop(a):
    """the definition, one sample at a time"""
    bins = [0] * 256
    for row in a:
        for s in row:
            bins[int(s)] += 1
    return bins


class CStats(C.Structure):
    _fields_ = [("count", C.c_uint32), ("min", C.c_uint32), ("max", C.c_uint32), ("zero", C.c_uint32), ("sum", C.c_uint64), ("sum2", C.c_uint64)]


@pytest.fixture(scope="module")
def c_hist(tmp_path_factory):
    """include/edge264_hist.h in a temporary library: the header compiles as C++ with every warning an error, alone and behind edge264_hip.h"""
    if not shutil.which("g++"):
        pytest.fail("no g++")
    d = tmp_path_factory.mktemp("hist_c")
    src = d / "hist_c.cpp"
    src.write_text('#include "edge264_hist.h"\n'
                   'extern "C" void hist_plane(const unsigned char *s, unsigned long stride, unsigned w, unsigned h, uint32_t *bin) { e264_hist_plane(s, stride, w, h, bin); }\n'
                   'extern "C" void hist_stats(const uint32_t *bin, E264HistStats *out) { e264_hist_stats(bin, out); }\n'
                   'extern "C" unsigned hist_quantile(const uint32_t *bin, uint32_t num, uint32_t den) { return e264_hist_quantile(bin, num, den); }\n'
                   'extern "C" int hist_version(void) { return EDGE264_HIST_VERSION; }\n'
                   'extern "C" int stats_sizeof(void) { return (int)sizeof(E264HistStats); }\n')
    lib = d / "libhist_c.so"
    flags = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include")]
    r = subprocess.run(flags + [str(src), "-o", str(lib)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    both = d / "both.cpp"
    both.write_text('#include "edge264_hip.h"\n#include "edge264_hist.h"\n'
                    'static_assert(sizeof(E264Hist) == 3072 && E264_HIST_VERSION == 1 && E264_HIST_VERSION == EDGE264_HIST_VERSION && E264_HIST_MAX_BATCH == 4096, "");\n'
                    'extern "C" void both(const unsigned char *s, E264Hist *out) { e264_hist_plane(s, 1, 1, 1, out->bin[2]); }\n')
    r = subprocess.run(flags + [str(both), "-o", str(d / "libboth.so")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(lib))
    L.hist_plane.restype = None
    L.hist_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_uint, C.c_void_p]
    L.hist_stats.restype = None
    L.hist_stats.argtypes = [C.c_void_p, C.POINTER(CStats)]
    L.hist_quantile.restype = C.c_uint
    L.hist_quantile.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    return L


def c_plane(L, a):
    """e264_hist_plane of a 2-D array (rows any distance apart)"""
    assert a.strides[1] == 1
    out = np.full(256, 7, np.uint32)
    L.hist_plane(a.ctypes.data, a.strides[0], a.shape[1], a.shape[0], out.ctypes.data)
    return out


def all_three(L, a):
    got = H.hist_plane(a)
    assert got.dtype == np.uint32 and got.shape == (256,)
    assert got.tolist() == c_plane(L, a).tolist() == plain_loop(a.tolist())
    return got


def one_hot(pairs):
    b = np.zeros(256, np.uint32)
    for v, n in pairs:
        b[v] += n
    return b.tolist()


def test_known_answers_numpy_c_and_plain_loop(c_hist):
    assert c_hist.hist_version() == H.HIST_VERSION == 1 and c_hist.stats_sizeof() == 32 and backend.HIST_MAX_BATCH == 4096
    w, h = 21, 6
    # a plane of zeros, a plane of 255s
    assert all_three(c_hist, np.zeros((h, w), np.uint8)).tolist() == one_hot([(0, w * h)])
    assert all_three(c_hist, np.full((h, w), 255, np.uint8)).tolist() == one_hot([(255, w * h)])
    # a 21 x 6 ramp: value x + y occurs once per (x, y) on its anti-diagonal
    ramp = (np.arange(w)[None, :] + np.arange(h)[:, None]).astype(np.uint8)
    want = one_hot([(x + y, 1) for y in range(h) for x in range(w)])
    assert want[0] == 1 and want[5] == 6 and want[20] == 6 and want[25] == 1 and want[26] == 0
    assert all_three(c_hist, ramp).tolist() == want
    # one sample moved by +-1: one count leaves its bin for the next
    base = np.full((h, w), 100, np.uint8)
    for i in (0, w * h - 1, 3 * w - 1, 3 * w):
        for step in (1, -1):
            b = base.copy()
            b.reshape(-1)[i] = 100 + step
            assert all_three(c_hist, b).tolist() == one_hot([(100, w * h - 1), (100 + step, 1)]), (i, step)
    # a strided view: the bytes between the rows do not count
    rng = np.random.default_rng(15)
    big = rng.integers(0, 256, (h, w + 11), dtype=np.uint8)
    view = big[:, 3:3 + w]
    assert not view.flags["C_CONTIGUOUS"]
    got = all_three(c_hist, view)
    assert got.tolist() == np.bincount(view.reshape(-1), minlength=256).tolist() and int(got.sum()) == w * h
    assert got.tolist() != H.hist_plane(big).tolist()
    # what has no record
    with pytest.raises(ValueError):
        H.hist_plane(ramp.astype(np.uint16))
    with pytest.raises(ValueError):
        H.hist_plane(ramp.reshape(-1))
    # frame_hist over a slot image in a padded layout
    v = D.frame_view(2, 1, geometry=dict(stride_Y=48, stride_C=48, plane_size_Y=48 * 16 + 7, plane_size_C=48 * 8))
    img = rng.integers(0, 256, 48 * 16 + 7 + 48 * 8, dtype=np.uint8)
    got = H.frame_hist(v, img)
    assert got.shape == (3, 256) and got.dtype == np.uint32 and got.sum(axis=1).tolist() == [32 * 16, 16 * 8, 16 * 8]
    assert all(got[p].tolist() == plain_loop(pl.tolist()) for p, pl in enumerate(D.view_planes(v, img)))
    # distance: the L1 distance of two bin arrays
    a, b = H.hist_plane(base), H.hist_plane(ramp)
    assert H.distance(a, a) == 0 and H.distance(a, b) == H.distance(b, a) == sum(abs(int(x) - int(y)) for x, y in zip(a, b)) == 2 * w * h


def c_stats(L, bins):
    b = np.ascontiguousarray(bins, np.uint32)
    out = CStats(9, 9, 9, 9, 9, 9)
    L.hist_stats(b.ctypes.data, C.byref(out))
    assert out.zero == 0
    return dict(count=out.count, min=out.min, max=out.max, sum=out.sum, sum2=out.sum2)


def test_stats_and_quantiles_against_numpy(c_hist):
    rng = np.random.default_rng(256)
    planes = [rng.integers(0, 256, (37, 53), dtype=np.uint8), rng.integers(16, 236, (8, 8), dtype=np.uint8), np.full((5, 7), 200, np.uint8),
              np.zeros((3, 3), np.uint8), np.full((2, 9), 255, np.uint8), (rng.integers(0, 2, (16, 16)) * 255).astype(np.uint8)]
    fractions = [(0, 1), (1, 1), (1, 2), (1, 4), (3, 4), (1, 100), (99, 100), (1, 1000), (5, 7)]
    for a in planes:
        bins = H.hist_plane(a)
        flat = np.sort(a.reshape(-1)).astype(np.int64)
        want = dict(count=flat.size, min=int(flat.min()), max=int(flat.max()), sum=int(flat.sum()), sum2=int((flat * flat).sum()))
        assert H.stats(bins) == want == c_stats(c_hist, bins)
        for num, den in fractions:
            k = -(-flat.size * num // den)  # the least number of samples that is num / den of them
            expect = int(flat[k - 1]) if k else 0
            got = H.quantile(bins, num, den)
            assert got == expect == c_hist.hist_quantile(np.ascontiguousarray(bins).ctypes.data, num, den), (num, den)
        assert H.quantile(bins, 1, 1) == want["max"] and H.quantile(bins, 0, 1) == 0
    # one occupied bin: every positive fraction names it
    one = np.zeros(256, np.uint32)
    one[77] = 12345
    assert [H.quantile(one, n, d) for n, d in fractions[1:]] == [77] * 8 == [c_hist.hist_quantile(one.ctypes.data, n, d) for n, d in fractions[1:]]
    assert H.quantile(one, 0, 1) == 0 == c_hist.hist_quantile(one.ctypes.data, 0, 1)
    assert H.stats(one) == dict(count=12345, min=77, max=77, sum=77 * 12345, sum2=77 * 77 * 12345) == c_stats(c_hist, one)
    # the largest plane's worth in one bin: the 64-bit members do not wrap
    full = np.zeros(256, np.uint32)
    full[255] = 65535 * 65535
    assert H.stats(full) == dict(count=65535 ** 2, min=255, max=255, sum=255 * 65535 ** 2, sum2=65025 * 65535 ** 2) == c_stats(c_hist, full)
    assert H.quantile(full, 1, 2) == 255 == c_hist.hist_quantile(full.ctypes.data, 1, 2)
    # an empty histogram
    empty = np.zeros(256, np.uint32)
    assert H.stats(empty) == dict(count=0, min=255, max=0, sum=0, sum2=0) == c_stats(c_hist, empty)
    assert H.quantile(empty, 1, 2) == 0 == c_hist.hist_quantile(empty.ctypes.data, 1, 2)
    with pytest.raises(ValueError):
        H.stats(np.zeros((3, 256), np.uint32))


def test_hist_kernel_body_on_the_host_under_sanitizers(tmp_path):
    """tests/emu/hist_asan.cpp: hist_thread run over grids of 1 to 768 threads in workgroups of 256, each workgroup's bins in a heap block of exactly their
    size and the plane in a heap block that ends with its last byte -- the sanitizers see no access outside either -- and the summed bins equal e264_hist_plane
    for 6 widths x 2 heights x 4 strides x 16 alignments x 21 contents x 2 grids"""
    exe = str(tmp_path / "hist_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "hist_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])
    m = re.search(r"hist_asan: (\d+) cases, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == 6 * 2 * 4 * 16 * 21 * 2, r.stdout[-500:]


def test_hist_kernel_resources(tmp_path):
    """e264_hist.hip cross-compiled for gfx950: the histogram kernel spills nothing, uses no scratch, no AGPRs and at most 128 VGPRs"""
    if not shutil.which(HIPCC):
        pytest.fail(f"no {HIPCC}: the cross-compiler is a tool of the build, not hardware")
    src = os.path.join(ROOT, "edge264_amd", "csrc", "e264_hist.hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "h.o"),
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
    hits = {k: v for k, v in kernels.items() if "e264_hist_kernel" in k}
    assert len(hits) == 1, sorted(kernels)
    r = next(iter(hits.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, r
    assert 0 < r["VGPRs"] <= 128 and r["AGPRs"] == 0, r


def test_library_surface_and_host_only_refusals():
    """the library loads without a GPU and has the entry points; what e264hip_hist_batch refuses before it looks at a device: a null device, n < 0, n = 4097
    -- EINVAL with a text, `out` untouched -- and n = 0 returns 0"""
    lib = backend.load_library()
    for name in ("e264hip_frame_hist", "e264hip_hist_batch"):
        assert hasattr(lib, name) and name in backend.EXPORTED_SYMBOLS
    out = np.full((2, 3, 256), 7, np.uint32)
    o = out.ctypes.data
    streams, slots, views = (C.c_void_p * 1)(None), (C.c_int * 1)(0), (backend.View * 1)(backend.as_view(D.frame_view(1, 1)))
    assert lib.e264hip_hist_batch(None, streams, slots, views, 1, o) == errno.EINVAL and "hist_batch" in backend.last_error()
    assert lib.e264hip_hist_batch(None, streams, slots, views, 0, o) == errno.EINVAL and "null device" in backend.last_error()
    fake = C.c_void_p(out.ctypes.data)  # a device pointer that is never followed: n is looked at first
    assert lib.e264hip_hist_batch(fake, streams, slots, views, -1, o) == errno.EINVAL and "n outside" in backend.last_error()
    assert lib.e264hip_hist_batch(fake, streams, slots, views, 4097, o) == errno.EINVAL and "n outside" in backend.last_error()
    assert lib.e264hip_hist_batch(fake, streams, slots, views, 0, o) == 0
    assert lib.e264hip_hist_batch(fake, None, None, None, 0, None) == 0
    assert lib.e264hip_frame_hist(None, 0, views, o) == errno.EINVAL and "null stream" in backend.last_error()
    assert (out == 7).all()


def test_front_hist_library():
    """edge264_amd/libedge264_frontdigest.so exports e264front_frame_hist (edge264_amd/frontend/front_hist.c) beside the digest's, the preview's and the diff's
    entry points, refuses null arguments and a view that is neither 0 nor 1 before it looks for the front library or the back end, and answers ENODEV where the
    front library is not to be found"""
    path = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = C.CDLL(path)
    lib.e264front_frame_hist.restype = C.c_int
    lib.e264front_frame_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.e264front_frame_digest, lib.e264front_frame_preview, lib.e264front_frame_diff, lib.e264front_digest_use  # (still there)
    out = np.full((3, 256), 7, np.uint32)
    frame = (C.c_char * 128)()
    o = out.ctypes.data
    assert lib.e264front_frame_hist(None, frame, 0, o) == errno.EINVAL
    assert lib.e264front_frame_hist(1, None, 0, o) == errno.EINVAL
    assert lib.e264front_frame_hist(1, frame, 0, None) == errno.EINVAL
    for v in (2, -1):
        assert lib.e264front_frame_hist(1, frame, v, o) == errno.EINVAL
    assert (out == 7).all()
    # without the front library: a copy of the library alone in a directory, in a process of its own (the binding is made once per process)
    code = ("import ctypes as C, shutil, sys, tempfile, os\n"
            "d = tempfile.mkdtemp()\n"
            "p = shutil.copy(sys.argv[1], os.path.join(d, 'libedge264_frontdigest.so'))\n"
            "os.environ.pop('E264_HIP_LIB', None)\n"
            "lib = C.CDLL(p)\n"
            "lib.e264front_frame_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]\n"
            "f = (C.c_char * 128)(); o = (C.c_char * 3072)()\n"
            "r = lib.e264front_frame_hist(1, f, 0, o)\n"
            "shutil.rmtree(d)\n"
            "print(r)\n")
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and int(r.stdout.strip()) == errno.ENODEV, (r.stdout, r.stderr[-2000:])
