"""The picture digest (include/edge264_hip.h, version 1) without a GPU: its definition in numpy and in C against known answers and each other,
the digest kernel's own body on the host under the address and undefined-behaviour sanitizers (tests/emu/digest_asan.cpp, a stand-alone program),
e264hip_view_check through the library, and the kernel's register budget from a cross-compilation.  tests/test_hip_digest.py runs the kernel."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, digest as D, packet as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def pattern(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return ((31 * x + 17 * y + ((x * y) >> 3) + 3) & 255).astype(np.uint8)


# the known answers of the definition: numpy, cross-checked against a plain loop for the small ones
KNOWN = [
    (np.zeros((2, 2), np.uint8), 0x108339fe6),
    (np.full((1, 1), 255, np.uint8), 0x100),
    (pattern(5, 3), 0x25912e0eac2),
    (pattern(80, 48), 0x3bfbed3c81f60),
    (pattern(1920, 1080), 0x7f0c334b333051a),
]


def plain_loop(plane):
    """the definition, one sample at a time"""
    def fmix32(h):
        h ^= h >> 16
        h = h * 0x85ebca6b & 0xffffffff
        h ^= h >> 13
        h = h * 0xc2b2ae35 & 0xffffffff
        return h ^ h >> 16
    return sum((int(s) + 1) * (fmix32(i) | 1) for i, s in enumerate(plane.reshape(-1))) & (1 << 64) - 1


def test_plane_digest_known_answers():
    for plane, want in KNOWN:
        assert D.plane_digest(plane) == want, plane.shape
    for plane, want in KNOWN[:4]:
        assert plain_loop(plane) == want, plane.shape
    # a view with strides is digested as the plane it shows
    big = np.random.default_rng(1).integers(0, 256, (50, 90), dtype=np.uint8)
    assert D.plane_digest(big[3:40, 7:60]) == D.plane_digest(big[3:40, 7:60].copy()) == plain_loop(big[3:40, 7:60])


@pytest.fixture(scope="module")
def c_digest(tmp_path_factory):
    """include/edge264_digest.h's e264_digest_plane in a temporary library: the header compiles as C++ with every warning an error"""
    if not shutil.which("g++"):
        pytest.fail("no g++")
    d = tmp_path_factory.mktemp("digest_c")
    src = d / "digest_c.cpp"
    src.write_text('#include "edge264_digest.h"\n'
                   'extern "C" unsigned long long digest_plane(const unsigned char *p, unsigned long stride, unsigned w, unsigned h) '
                   '{ return e264_digest_plane(p, stride, w, h); }\n'
                   'extern "C" int digest_version(void) { return EDGE264_DIGEST_VERSION; }\n')
    lib = d / "libdigest_c.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(lib)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(lib))
    L.digest_plane.restype = C.c_uint64
    L.digest_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_uint]
    return L


def test_c_header_equals_numpy(c_digest):
    assert c_digest.digest_version() == D.DIGEST_VERSION == 1
    for plane, want in KNOWN:
        a = np.ascontiguousarray(plane)
        assert c_digest.digest_plane(a.ctypes.data, a.shape[1], a.shape[1], a.shape[0]) == want, plane.shape
    rng = np.random.default_rng(264)
    for k in range(200):
        w, h = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        stride = w + (0, 1, 3, 16)[k % 4]
        buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)  # random bytes in the padding too
        assert c_digest.digest_plane(buf.ctypes.data, stride, w, h) == D.plane_digest(buf[:, :w]), (w, h, stride)


def test_digest_kernel_body_on_the_host_under_sanitizers(tmp_path):
    """tests/emu/digest_asan.cpp: digest_thread summed over grids of 1 to 1792 threads equals e264_digest_plane for 17 widths x 4 heights x 4 strides x
    16 alignments, every plane in a heap block that ends with its last byte -- and the sanitizers see no load outside the block"""
    exe = str(tmp_path / "digest_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "digest_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])
    m = re.search(r"digest_asan: (\d+) cases, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == 17 * 4 * 4 * 16 * 5, r.stdout[-500:]


def view_of(offset, stride, width, height):
    return dict(offset=[offset] * 3, stride=[stride] * 3, width=[width] * 3, height=[height] * 3)


def test_view_check():
    """e264hip_view_check through the library (which loads without a GPU)"""
    ok = view_of(100, 64, 48, 10)
    extent = 100 + 9 * 64 + 48
    assert backend.view_check(ok, extent) == 0
    assert backend.view_check(ok, extent - 1) == errno.EINVAL and "leaves the slot" in backend.last_error()
    assert backend.view_check(view_of(101, 64, 48, 10), extent) == errno.EINVAL  # one more
    assert backend.view_check(view_of(0, 64, 0, 10), 1 << 20) == errno.EINVAL and backend.last_error()
    assert backend.view_check(view_of(0, 64, 48, 0), 1 << 20) == errno.EINVAL and backend.last_error()
    assert backend.view_check(view_of(0, 47, 48, 10), 1 << 20) == errno.EINVAL and "stride" in backend.last_error()
    # refused, not wrapped: the sums are 64-bit
    assert backend.view_check(view_of(0xffffffff, 64, 48, 10), extent) == errno.EINVAL
    assert backend.view_check(view_of(0xffffffff, 64, 48, 10), 0xffffffff) == errno.EINVAL
    assert backend.view_check(view_of(0, 0xffffffff, 48, 65535), 1 << 20) == errno.EINVAL
    assert backend.view_check(view_of(0, 0xffffffff, 48, 65535), 0xffffffff) == errno.EINVAL
    assert backend.view_check(view_of(0, 0xffffffff, 48, 65535), 65534 * 0xffffffff + 48) == 0  # (what it really needs)
    # one bad plane is enough, whichever it is
    for p in range(3):
        v = view_of(100, 64, 48, 10)
        v["offset"][p] += 1
        assert backend.view_check(v, extent) == errno.EINVAL and ("Y", "Cb", "Cr")[p] in backend.last_error()
    assert backend.load_library().e264hip_view_check(None, 100) == errno.EINVAL


def test_frame_view():
    """digest.frame_view is the reference's layout: what an Edge264Frame says about a slot"""
    g = P.frame_geometry(5, 3)
    v = D.frame_view(5, 3)
    assert v == dict(offset=[0, g["plane_size_Y"], g["plane_size_Y"] + g["stride_C"] // 2], stride=[g["stride_Y"], g["stride_C"], g["stride_C"]],
                     width=[80, 40, 40], height=[48, 24, 24])
    assert backend.view_check(v, P.frame_bytes(5, 3)) == 0 and backend.view_check(v, P.frame_bytes(5, 3) - 1) == errno.EINVAL  # Cr ends the slot
    c = D.frame_view(5, 3, crop=(2, 6, 2, 10))
    assert c["offset"][0] == 2 * g["stride_Y"] + 2 and c["offset"][1] == g["plane_size_Y"] + g["stride_C"] + 1 and c["offset"][1] & 1
    assert c["width"] == [72, 36, 36] and c["height"] == [36, 18, 18]
    slot = np.random.default_rng(3).integers(0, 256, P.frame_bytes(5, 3), dtype=np.uint8)
    y = slot[:g["plane_size_Y"]].reshape(48, 80)
    ch = slot[g["plane_size_Y"]:].reshape(24, 80)
    assert D.frame_digest(c, slot) == (D.plane_digest(y[2:38, 2:74]), D.plane_digest(ch[1:19, 1:37]), D.plane_digest(ch[1:19, 41:77]))
    with pytest.raises(ValueError):
        D.frame_view(1, 1, crop=(8, 8, 0, 0))


def test_digest_kernel_resources(tmp_path):
    """e264_digest.hip cross-compiled for gfx950: the digest kernel spills nothing and uses no scratch"""
    if not shutil.which(HIPCC):
        pytest.fail(f"no {HIPCC}: the cross-compiler is a tool of the build, not hardware")
    src = os.path.join(ROOT, "edge264_amd", "csrc", "e264_digest.hip")
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
    hits = {k: v for k, v in kernels.items() if "e264_digest_kernel" in k}
    assert len(hits) == 1, sorted(kernels)
    r = next(iter(hits.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, r


def test_front_digest_library():
    """edge264_amd/libedge264_frontdigest.so (e264front_frame_digest, edge264_amd/frontend/front_digest.c) is built by __graft_entry__.build() on a machine
    without the reference tree too, and refuses null arguments before it looks for the front library or the back end"""
    path = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = C.CDLL(path)
    lib.e264front_frame_digest.restype = C.c_int
    lib.e264front_frame_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.e264front_digest_use.restype = C.c_int
    lib.e264front_digest_use.argtypes = [C.c_void_p, C.c_void_p]
    out = (C.c_uint64 * 3)()
    frame = (C.c_char * 128)()
    assert lib.e264front_frame_digest(None, frame, 0, out) == errno.EINVAL
    assert lib.e264front_frame_digest(1, None, 0, out) == errno.EINVAL
    assert lib.e264front_frame_digest(1, frame, 0, None) == errno.EINVAL
    assert lib.e264front_frame_digest(1, frame, 2, out) == errno.EINVAL
    assert lib.e264front_digest_use(None, 1) == errno.EINVAL and lib.e264front_digest_use(1, None) == errno.EINVAL
