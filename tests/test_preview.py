"""The reduced preview (include/edge264_hip.h, version 1) without a GPU: its definition in numpy, in C and in a plain loop against known answers and each
other, e264hip_preview_bytes through the library, the preview kernel's own body on the host under the address and undefined-behaviour sanitizers
(tests/emu/preview_asan.cpp, a stand-alone program), the kernel's register budget from a cross-compilation, and the front library's entry point.
tests/test_hip_preview.py runs the kernel."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, digest as D, preview as PV

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# the known answers of the definition (k, plane, preview), worked out by hand
KNOWN = [
    (1, [[0, 1], [2, 3]], [[2]]),                            # (6 + 2) >> 2
    (1, [[0, 0], [0, 1]], [[0]]),                            # (1 + 2) >> 2
    (1, [[0, 1], [1, 0]], [[1]]),                            # (2 + 2) >> 2: half rounds up
    (1, [[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[3, 5], [8, 9]]),  # the last column and row repeat: (3 + 3 + 6 + 6 + 2) >> 2, (7 + 8 + 7 + 8 + 2) >> 2, (4 * 9 + 2) >> 2
    (1, [[255]], [[255]]),
    (2, [[255]], [[255]]),
    (3, [[255]], [[255]]),
]


def plain_loop(plane, k):
    """the definition, one sample at a time"""
    h, w = len(plane), len(plane[0])
    f = 1 << k
    ow, oh = (w + f - 1) >> k, (h + f - 1) >> k
    return [[(sum(int(plane[min(f * Y + dy, h - 1)][min(f * X + dx, w - 1)]) for dy in range(f) for dx in range(f)) + (1 << (2 * k - 1))) >> (2 * k)
             for X in range(ow)] for Y in range(oh)]


@pytest.fixture(scope="module")
def c_preview(tmp_path_factory):
    """include/edge264_preview.h in a temporary library: the header compiles as C++ with every warning an error"""
    if not shutil.which("g++"):
        pytest.fail("no g++")
    d = tmp_path_factory.mktemp("preview_c")
    src = d / "preview_c.cpp"
    src.write_text('#include "edge264_preview.h"\n'
                   'extern "C" void preview_plane(const unsigned char *p, unsigned long stride, unsigned w, unsigned h, int k, unsigned char *dst, unsigned long dst_stride) '
                   '{ e264_preview_plane(p, stride, w, h, k, dst, dst_stride); }\n'
                   'extern "C" int preview_dims(unsigned w, unsigned h, int k, unsigned *ow, unsigned *oh) { return e264_preview_dims(w, h, k, ow, oh); }\n'
                   'extern "C" int preview_version(void) { return EDGE264_PREVIEW_VERSION; }\n')
    lib = d / "libpreview_c.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(lib)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(lib))
    L.preview_plane.restype = None
    L.preview_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_ulong]
    L.preview_dims.argtypes = [C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    return L


def c_plane_preview(L, buf, stride, w, h, k, dst_pad=0):
    """e264_preview_plane of the w x h plane at the start of buf; the destination's rows dst_pad bytes apart from tight, pre-filled: only the preview is written"""
    ow, oh = C.c_uint(), C.c_uint()
    assert L.preview_dims(w, h, k, C.byref(ow), C.byref(oh)) == 1
    ow, oh = ow.value, oh.value
    out = np.full((oh, ow + dst_pad), 0xa5, np.uint8)
    L.preview_plane(buf.ctypes.data, stride, w, h, k, out.ctypes.data, ow + dst_pad)
    assert (out[:, ow:] == 0xa5).all()
    return out[:, :ow]


def test_known_answers_numpy_c_and_plain_loop(c_preview):
    assert c_preview.preview_version() == PV.PREVIEW_VERSION == 1
    for k, plane, want in KNOWN:
        a = np.array(plane, np.uint8)
        assert PV.plane_preview(a, k).tolist() == want, (k, plane)
        assert c_plane_preview(c_preview, a, a.shape[1], a.shape[1], a.shape[0], k, dst_pad=3).tolist() == want, (k, plane)
        assert plain_loop(plane, k) == want, (k, plane)
    # a view with strides is reduced as the plane it shows
    big = np.random.default_rng(1).integers(0, 256, (50, 90), dtype=np.uint8)
    for k in (1, 2, 3):
        got = PV.plane_preview(big[3:40, 7:60], k)
        assert got.dtype == np.uint8 and got.shape == ((37 + (1 << k) - 1) >> k, (53 + (1 << k) - 1) >> k)
        assert got.tolist() == PV.plane_preview(big[3:40, 7:60].copy(), k).tolist() == plain_loop(big[3:40, 7:60].tolist(), k)
    # what has no preview
    one = np.zeros((1, 1), np.uint8)
    n = C.c_uint(77)
    for k in (0, 4, -1):
        with pytest.raises(ValueError):
            PV.plane_preview(one, k)
        assert c_preview.preview_dims(1, 1, k, C.byref(n), C.byref(n)) == 0 and n.value == 77
    assert c_preview.preview_dims(0, 1, 1, C.byref(n), C.byref(n)) == 0 and c_preview.preview_dims(1, 0, 1, C.byref(n), C.byref(n)) == 0


def test_c_header_equals_numpy(c_preview):
    rng = np.random.default_rng(264)
    for i in range(200):
        w, h = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        k = 1 + i % 3
        stride = w + (0, 1, 3, 16)[i % 4]
        buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)  # random bytes in the padding too
        assert np.array_equal(c_plane_preview(c_preview, buf, stride, w, h, k, dst_pad=i % 5), PV.plane_preview(buf[:, :w], k)), (w, h, k, stride)


def view_of(offset, stride, width, height):
    return dict(offset=[offset] * 3, stride=[stride] * 3, width=list(width) if isinstance(width, (list, tuple)) else [width] * 3,
                height=list(height) if isinstance(height, (list, tuple)) else [height] * 3)


def test_preview_bytes_through_the_library():
    """e264hip_preview_bytes (host only: the library loads without a GPU): sizes and every refusal"""
    lib = backend.load_library()
    v1080 = D.frame_view(120, 68, crop=(0, 0, 0, 8))  # 1920 x 1080
    assert v1080["width"] == [1920, 960, 960] and v1080["height"] == [1080, 540, 540]
    assert backend.preview_bytes(v1080, 3) == 240 * 135 + 2 * 120 * 68 == PV.preview_bytes(v1080, 3)
    assert backend.preview_bytes(v1080, 2) == 480 * 270 + 2 * 240 * 135 == PV.preview_bytes(v1080, 2)
    assert backend.preview_bytes(v1080, 1) == 960 * 540 + 2 * 480 * 270 == PV.preview_bytes(v1080, 1)
    dims = (C.c_uint16 * 6)()
    assert lib.e264hip_preview_bytes(C.byref(backend.as_view(v1080)), 3, dims) == 48720 and list(dims) == [240, 135, 120, 68, 120, 68]
    assert backend.preview_dims(v1080, 2) == [(480, 270), (240, 135), (240, 135)]
    # sizes that are no multiple of the factor round up, each plane on its own; the largest plane there is
    odd = view_of(0, 100, [17, 9, 9], [9, 5, 5])
    assert [backend.preview_bytes(odd, k) for k in (1, 2, 3)] == [9 * 5 + 2 * 5 * 3, 5 * 3 + 2 * 3 * 2, 3 * 2 + 2 * 2 * 1]
    assert backend.preview_bytes(view_of(0, 65535, 1, 1), 3) == 3
    assert backend.preview_bytes(view_of(0, 65535, 65535, 65535), 1) == 3 * 32768 * 32768
    for w, h in ((1, 1), (7, 3), (64, 64), (65, 63)):
        for k in (1, 2, 3):
            assert backend.preview_bytes(view_of(0, 100, w, h), k) == 3 * PV.plane_preview(np.zeros((h, w), np.uint8), k).size == PV.preview_bytes(view_of(0, 100, w, h), k)
    # refusals: 0, and dims untouched
    dims = (C.c_uint16 * 6)(*[7] * 6)
    assert lib.e264hip_preview_bytes(None, 3, dims) == 0
    for k in (0, 4, -1, 1 << 20):
        assert lib.e264hip_preview_bytes(C.byref(backend.as_view(v1080)), k, dims) == 0, k
        assert backend.preview_bytes(v1080, k) == 0
    for p in range(3):
        for field in ("width", "height"):
            bad = backend.as_view(v1080)
            setattr(bad.plane[p], field, 0)
            assert lib.e264hip_preview_bytes(C.byref(bad), 3, dims) == 0, (p, field)
    assert list(dims) == [7] * 6
    assert backend.preview_bytes(None, 3) == 0
    with pytest.raises(ValueError):
        backend.preview_dims(v1080, 0)
    with pytest.raises(ValueError):
        PV.preview_bytes(v1080, 4)


def test_preview_kernel_body_on_the_host_under_sanitizers(tmp_path):
    """tests/emu/preview_asan.cpp: preview_thread run over grids of 1 to 768 threads equals e264_preview_plane for 14 widths x 5 heights x 4 strides x
    16 alignments x 3 reductions, every plane in a heap block that ends with its last byte and the preview in a block of exactly its size -- the sanitizers
    see no access outside either block, and every byte of the preview is stored exactly once"""
    exe = str(tmp_path / "preview_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "preview_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])
    m = re.search(r"preview_asan: (\d+) cases, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == 14 * 5 * 4 * 16 * 3 * 4, r.stdout[-500:]


def test_preview_kernel_resources(tmp_path):
    """e264_preview.hip cross-compiled for gfx950: the preview kernel spills nothing and uses no scratch"""
    if not shutil.which(HIPCC):
        pytest.fail(f"no {HIPCC}: the cross-compiler is a tool of the build, not hardware")
    src = os.path.join(ROOT, "edge264_amd", "csrc", "e264_preview.hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "p.o"),
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
    hits = {k: v for k, v in kernels.items() if "e264_preview_kernel" in k}
    assert len(hits) == 1, sorted(kernels)
    r = next(iter(hits.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, r


def test_front_preview_library():
    """edge264_amd/libedge264_frontdigest.so exports e264front_frame_preview (edge264_amd/frontend/front_preview.c) beside e264front_frame_digest, and refuses
    null arguments, a view that is neither 0 nor 1 and k outside 1..3 before it looks for the front library or the back end"""
    path = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = C.CDLL(path)
    lib.e264front_frame_preview.restype = C.c_int
    lib.e264front_frame_preview.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint16)]
    lib.e264front_frame_digest  # (still there)
    out = (C.c_uint8 * 64)()
    dims = (C.c_uint16 * 6)()
    frame = (C.c_char * 128)()
    assert lib.e264front_frame_preview(None, frame, 0, 3, out, 64, dims) == errno.EINVAL
    assert lib.e264front_frame_preview(1, None, 0, 3, out, 64, dims) == errno.EINVAL
    assert lib.e264front_frame_preview(1, frame, 0, 3, None, 64, dims) == errno.EINVAL
    assert lib.e264front_frame_preview(1, frame, 2, 3, out, 64, dims) == errno.EINVAL
    for k in (0, 4, -1):
        assert lib.e264front_frame_preview(1, frame, 0, k, out, 64, None) == errno.EINVAL
