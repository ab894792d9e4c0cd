"""The block statistics map (include/edge264_hip.h, version 1) without a GPU: its definition in numpy, in C and in a plain loop against known answers and each
other, the invariants against the histogram record and the block difference map, the kernel's own body on the host under the address and undefined-behaviour
sanitizers (tests/emu/blockstat_asan.cpp, a stand-alone program), the kernel's register budget from a cross-compilation, the library's and the front library's
entry points, and the refusals that need no device.  tests/test_hip_blockstat.py runs the kernel.  Everything is compared for equality: there is no tolerance
anywhere."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from edge264_amd import backend, blockdiff as BD, blockstat as BS, digest as D, hist as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SIZES = (1, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 129)
KS = (3, 4, 5, 6)
FIELDS = ("sum", "sumsq", "gh", "gv")


def plain_loop(a, k):
    """the definition, one sample at a time: [[(sum, sumsq, gh, gv)]] of bh rows of bw blocks"""
    h, w = len(a), len(a[0])
    bs = 1 << k
    bw, bh = (w + bs - 1) >> k, (h + bs - 1) >> k
    out = [[[0, 0, 0, 0] for _ in range(bw)] for _ in range(bh)]
    for y in range(h):
        for x in range(w):
            s = a[y][x]
            r = out[y >> k][x >> k]
            r[0] += s
            r[1] += s * s
            if x + 1 < w:
                r[2] += abs(a[y][x + 1] - s)
            if y + 1 < h:
                r[3] += abs(a[y + 1][x] - s)
    return [[tuple(r) for r in row] for row in out]


def as_lists(m):
    return [[tuple(int(r[f]) for f in FIELDS) for r in row] for row in m]


class CBlockStat(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in FIELDS]


@pytest.fixture(scope="module")
def c_blockstat(tmp_path_factory):
    """include/edge264_blockstat.h in a temporary library: the header compiles as C and as C++17 with every warning an error, alone and behind edge264_hip.h"""
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.fail("no gcc / g++")
    d = tmp_path_factory.mktemp("blockstat_c")
    body = ('{ext} void bs_plane(const unsigned char *s, unsigned long stride, unsigned w, unsigned h, int k, E264BlockStat *out) '
            '{{ e264_blockstat_plane(s, stride, w, h, k, out); }}\n'
            '{ext} int bs_dims(unsigned w, unsigned h, int k, unsigned *bw, unsigned *bh) {{ return e264_blockstat_dims(w, h, k, bw, bh); }}\n'
            '{ext} int bs_version(void) {{ return EDGE264_BLOCKSTAT_VERSION; }}\n'
            '{ext} int bs_sizeof(void) {{ return (int)sizeof(E264BlockStat); }}\n')
    check = ('{sa}(sizeof(E264BlockStat) == 16 && E264_BLOCKSTAT_VERSION == EDGE264_BLOCKSTAT_VERSION && E264_BLOCKSTAT_MAX_BATCH == 4096 && '
             'E264_BLOCKSTAT_MAX_BYTES == (1u << 28), "");\n')
    inc = "-I" + os.path.join(ROOT, "include")
    libs = {}
    for lang, cc, std, ext, sa in (("cpp", "g++", "-std=c++17", 'extern "C"', "static_assert"), ("c", "gcc", "-std=c11", "", "_Static_assert")):
        flags = [cc, std, "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", inc]
        alone = d / f"alone.{lang}"
        alone.write_text('#include "edge264_blockstat.h"\n' + body.format(ext=ext))
        lib = d / f"libblockstat_{lang}.so"
        r = subprocess.run(flags + [str(alone), "-o", str(lib)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        both = d / f"both.{lang}"
        both.write_text('#include "edge264_hip.h"\n#include "edge264_blockstat.h"\n' + check.format(sa=sa) + body.format(ext=ext))
        r = subprocess.run(flags + [str(both), "-o", str(d / f"libboth_{lang}.so")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        L = C.CDLL(str(lib))
        L.bs_plane.restype = None
        L.bs_plane.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_uint, C.c_int, C.POINTER(CBlockStat)]
        L.bs_dims.argtypes = [C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        libs[lang] = L
    return libs


def c_plane(L, a, k):
    """e264_blockstat_plane of a 2-D array (rows any distance apart), with a guard record behind the map"""
    assert a.strides[1] == 1
    bw, bh = C.c_uint(), C.c_uint()
    assert L.bs_dims(a.shape[1], a.shape[0], k, C.byref(bw), C.byref(bh)) == 1
    n = bw.value * bh.value
    out = (CBlockStat * (n + 1))()
    guard = (0x5a5a5a5a, 0xa5a5a5a5, 0x12345678, 0x9abcdef0)
    for f, v in zip(FIELDS, guard):
        setattr(out[n], f, v)
    L.bs_plane(a.ctypes.data, a.strides[0], a.shape[1], a.shape[0], k, out)
    assert tuple(getattr(out[n], f) for f in FIELDS) == guard
    return [[tuple(getattr(out[y * bw.value + x], f) for f in FIELDS) for x in range(bw.value)] for y in range(bh.value)]


def all_three(libs, a, k):
    got = BS.plane_blockstat(a, k)
    bw, bh = BS.blockstat_dims(a.shape[1], a.shape[0], k)
    assert got.shape == (bh, bw) and got.dtype == BS.BLOCKSTAT_DTYPE
    assert as_lists(got) == c_plane(libs["cpp"], a, k) == c_plane(libs["c"], a, k) == plain_loop(a.tolist(), k), (a.shape, k)
    return got


def rec(m, Y, X):
    return tuple(int(m[Y, X][f]) for f in FIELDS)


def test_constants_and_dims(c_blockstat):
    L = c_blockstat["cpp"]
    assert L.bs_version() == c_blockstat["c"].bs_version() == BS.BLOCKSTAT_VERSION == 1
    assert L.bs_sizeof() == c_blockstat["c"].bs_sizeof() == 16 == BS.BLOCKSTAT_DTYPE.itemsize == backend.BLOCKSTAT_DTYPE.itemsize
    assert BS.BLOCKSTAT_DTYPE == backend.BLOCKSTAT_DTYPE and backend.BLOCKSTAT_MAX_BATCH == 4096 and backend.BLOCKSTAT_MAX_BYTES == 1 << 28
    assert BS.BLOCKSTAT_DTYPE.names == FIELDS
    bw, bh = C.c_uint(77), C.c_uint(77)
    for k in (-1, 0, 2, 7):
        assert L.bs_dims(16, 16, k, C.byref(bw), C.byref(bh)) == 0 and (bw.value, bh.value) == (77, 77)
        with pytest.raises(ValueError):
            BS.blockstat_dims(16, 16, k)
    assert L.bs_dims(0, 16, 4, C.byref(bw), C.byref(bh)) == 0 and L.bs_dims(16, 0, 4, C.byref(bw), C.byref(bh)) == 0
    for k in KS:
        for w in SIZES:
            for h in (1, 64, 65):
                assert L.bs_dims(w, h, k, C.byref(bw), C.byref(bh)) == 1
                assert (bw.value, bh.value) == BS.blockstat_dims(w, h, k) == BD.blockdiff_dims(w, h, k) == (-(-w // (1 << k)), -(-h // (1 << k)))
                n = BS.counts(w, h, k)
                assert n.shape == (bh.value, bw.value) and int(n.sum()) == w * h and n.max() <= 1 << 2 * k and n.min() >= 1
    with pytest.raises(ValueError):
        BS.plane_blockstat(np.zeros((4, 4), np.uint16), 3)
    with pytest.raises(ValueError):
        BS.plane_blockstat(np.zeros(16, np.uint8), 3)


@pytest.mark.parametrize("k", KS)
def test_lone_255_at_block_corners_and_view_edges(c_blockstat, k):
    """a lone 255 in zeros: at the four corners of an inner block, at the view's last column and at its last row.  Its own block gets sum and sumsq and the
    pairs to its right and below it; the pair to its LEFT goes to the block of the sample left of it and the pair ABOVE it to the block of the sample above
    it -- the NEIGHBOURING blocks where the 255 sits at its block's left or top edge; a pair that would leave the view does not exist"""
    bs = 1 << k
    w, h = 3 * bs + 5, 3 * bs + 3  # three whole blocks and a partial one in each direction
    bw, bh = BS.blockstat_dims(w, h, k)
    assert (bw, bh) == (4, 4)
    X = Y = 1
    x0, y0, x1, y1 = bs * X, bs * Y, bs * X + bs - 1, bs * Y + bs - 1
    spots = [(x0, y0), (x1, y0), (x0, y1), (x1, y1), (w - 1, y0 + 2), (x0 + 2, h - 1), (w - 1, h - 1), (0, 0)]
    for x, y in spots:
        a = np.zeros((h, w), np.uint8)
        a[y, x] = 255
        got = all_three(c_blockstat, a, k)
        want = np.zeros((bh, bw), BS.BLOCKSTAT_DTYPE)
        want[y >> k, x >> k]["sum"] = 255
        want[y >> k, x >> k]["sumsq"] = 65025
        if x + 1 < w:
            want[y >> k, x >> k]["gh"] += 255           # the pair to its right: its own block, also when x + 1 lies in the next
        if x > 0:
            want[y >> k, (x - 1) >> k]["gh"] += 255     # the pair to its left: the left sample's block
        if y + 1 < h:
            want[y >> k, x >> k]["gv"] += 255
        if y > 0:
            want[(y - 1) >> k, x >> k]["gv"] += 255
        assert (got == want).all(), (k, x, y, np.argwhere(got != want).tolist())
    # spelled out for the top-left corner of block (1, 1): the left and the upper neighbour hold the pairs into it
    a = np.zeros((h, w), np.uint8)
    a[y0, x0] = 255
    m = BS.plane_blockstat(a, k)
    assert rec(m, 1, 1) == (255, 65025, 255, 255) and rec(m, 1, 0) == (0, 0, 255, 0) and rec(m, 0, 1) == (0, 0, 0, 255) and rec(m, 0, 0) == (0, 0, 0, 0)
    # ... and for the view's last column and last row: no pair to the right / below
    a = np.zeros((h, w), np.uint8)
    a[y0 + 2, w - 1] = 255
    m = BS.plane_blockstat(a, k)
    assert rec(m, 1, 3) == (255, 65025, 255, 510) and int(m["gh"].sum()) == 255  # (w - 1 = 3 b + 4: the sample left of it lies in the same partial block)
    a = np.zeros((h, w), np.uint8)
    a[h - 1, x0 + 2] = 255
    m = BS.plane_blockstat(a, k)
    assert rec(m, 3, 1) == (255, 65025, 510, 255) and int(m["gv"].sum()) == 255


@pytest.mark.parametrize("k", KS)
def test_extremes_one_column_one_row(c_blockstat, k):
    """a 0/255 checkerboard gives the largest gh and gv a block can hold, an all-255 block the largest sum and sumsq; planes of one column and of one row have
    no horizontal / vertical pair at all"""
    bs = 1 << k
    yy, xx = np.mgrid[0:2 * bs + 1, 0:2 * bs + 1]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    m = all_three(c_blockstat, board, k)
    n = bs * bs
    # block (0, 0): every sample has a right and a lower neighbour inside the view, each pair 255
    assert rec(m, 0, 0) == (255 * (n // 2), 65025 * (n // 2), 255 * n, 255 * n)
    # the corner block is the single sample (2 b, 2 b), a 0: no pair; the blocks of the last column / row have pairs in one direction only
    half = bs // 2
    assert rec(m, 2, 2) == (0, 0, 0, 0) and rec(m, 0, 2) == (255 * half, 65025 * half, 0, 255 * bs) and rec(m, 2, 0) == (255 * half, 65025 * half, 255 * bs, 0)
    full = np.full((bs, bs), 255, np.uint8)
    m = all_three(c_blockstat, full, k)
    assert as_lists(m) == [[(255 * n, 65025 * n, 0, 0)]]
    if k == 6:
        assert 255 * n == 4096 * 255 < 1 << 21 and 65025 * n == 4096 * 65025 < 1 << 29
        board64 = board[:64, :64].copy()
        m = all_three(c_blockstat, board64, 6)
        assert rec(m, 0, 0) == (255 * 2048, 65025 * 2048, 255 * 64 * 63, 255 * 64 * 63)
    rng = np.random.default_rng(k)
    col = rng.integers(0, 256, (2 * bs + 3, 1), dtype=np.uint8)
    m = all_three(c_blockstat, col, k)
    assert m.shape == (3, 1) and not m["gh"].any() and int(m["gv"].sum()) == int(np.abs(np.diff(col[:, 0].astype(int))).sum())
    row = rng.integers(0, 256, (1, 2 * bs + 3), dtype=np.uint8)
    m = all_three(c_blockstat, row, k)
    assert m.shape == (1, 3) and not m["gv"].any() and int(m["gh"].sum()) == int(np.abs(np.diff(row[0].astype(int))).sum())
    one = np.array([[200]], np.uint8)
    assert as_lists(all_three(c_blockstat, one, k)) == [[(200, 40000, 0, 0)]]


@pytest.mark.parametrize("k", KS)
def test_numpy_c_and_plain_loop_and_the_invariants(c_blockstat, k):
    """every w, h of SIZES, random planes: numpy and C agree (and the plain loop, on a subset: it is slow); per plane the sums of sum and sumsq are the
    histogram record's first and second moments; the block difference map against zeros has sad == sum and sse == sumsq record for record; the sums of gh and
    gv are the plane's total variation; n sumsq - sum^2 >= 0 with equality exactly for flat blocks"""
    rng = np.random.default_rng(170 + k)
    v = np.arange(256, dtype=np.uint64)
    for w in SIZES:
        for h in SIZES:
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            if (w + h) % 3 == 0:
                a[: h // 2 + 1, : w // 2 + 1] = int(rng.integers(0, 256))  # a flat region: whole flat blocks where it covers some
            if (w, h) in ((129, 129), (65, 33), (17, 9), (1, 1), (8, 64)) or w == h:
                got = all_three(c_blockstat, a, k)
            else:
                got = BS.plane_blockstat(a, k)
                assert as_lists(got) == c_plane(c_blockstat["cpp"], a, k), (w, h)
            bins = H.hist_plane(a).astype(np.uint64)
            assert int(got["sum"].sum(dtype=np.uint64)) == int((v * bins).sum()) == H.stats(bins)["sum"]
            assert int(got["sumsq"].sum(dtype=np.uint64)) == int((v * v * bins).sum()) == H.stats(bins)["sum2"]
            zero = BD.blockdiff_plane(a, np.zeros_like(a), k)
            assert (zero["sad"] == got["sum"]).all() and (zero["sse"] == got["sumsq"]).all()
            s = a.astype(np.int64)
            assert int(got["gh"].sum(dtype=np.uint64)) == int(np.abs(np.diff(s, axis=1)).sum()) and int(got["gv"].sum(dtype=np.uint64)) == int(np.abs(np.diff(s, axis=0)).sum())
            n = BS.counts(w, h, k)
            num = n * got["sumsq"].astype(np.int64) - got["sum"].astype(np.int64) ** 2
            assert (num >= 0).all()
            bs = 1 << k
            truly_flat = np.array([[len(np.unique(a[Y * bs:Y * bs + bs, X * bs:X * bs + bs])) == 1 for X in range(got.shape[1])] for Y in range(got.shape[0])])
            assert ((num == 0) == truly_flat).all() and (BS.flat(got, w, h, k) == truly_flat).all()
            assert np.array_equal(BS.mean(got, w, h, k), got["sum"] / n) and (BS.variance(got, w, h, k) >= 0).all()
            assert ((BS.variance(got, w, h, k) == 0) == truly_flat).all()


def test_total_variation_is_independent_of_k():
    """a pair goes to one block only: the sums of gh and of gv over the maps at k = 3, 4, 5, 6 are equal (and so are those of sum and sumsq)"""
    rng = np.random.default_rng(3456)
    for w, h in ((129, 65), (64, 64), (17, 9), (1, 70), (70, 1), (33, 130)):
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        totals = {tuple(int(BS.plane_blockstat(a, k)[f].sum(dtype=np.uint64)) for f in FIELDS) for k in KS}
        assert len(totals) == 1, (w, h, totals)


def test_c_header_equals_numpy_on_strided_planes(c_blockstat):
    """random planes in rows of other lengths, random bytes in the padding; frame_blockstat over a slot image in a padded layout"""
    rng = np.random.default_rng(265)
    for i in range(120):
        w, h, k = int(rng.integers(1, 140)), int(rng.integers(1, 140)), KS[i % 4]
        A = rng.integers(0, 256, (h, w + (0, 1, 3, 16)[(i // 4) % 4]), dtype=np.uint8)
        assert c_plane(c_blockstat["c"], A[:, :w], k) == as_lists(BS.plane_blockstat(A[:, :w], k)), (w, h, k)
    v = D.frame_view(2, 1, geometry=dict(stride_Y=48, stride_C=48, plane_size_Y=48 * 16 + 7, plane_size_C=48 * 8))
    img = rng.integers(0, 256, 48 * 16 + 7 + 48 * 8, dtype=np.uint8)
    got = BS.frame_blockstat(v, img, 3)
    assert [m.shape for m in got] == [(2, 4), (1, 2), (1, 2)]
    for m, p in zip(got, D.view_planes(v, img)):
        assert (m == BS.plane_blockstat(p, 3)).all() and int(m["sum"].sum()) == int(p.astype(np.int64).sum())
    flat_bytes = np.concatenate([m.reshape(-1).view(np.uint8) for m in got])
    back = BS.split_map(flat_bytes, [(4, 2), (2, 1), (2, 1)])
    assert all((x == y).all() for x, y in zip(back, got))


def test_bars_mean_variance_flat():
    """the letterbox / pillarbox use: a 96 x 64 picture with 16 black rows on top, 24 at the bottom (one and a half block rows: only one whole), and, between
    them, 16 black columns at the left and 32 at the right; bars at another level than the first do not count; a picture without bars; a flat picture"""
    rng = np.random.default_rng(11)
    w, h, k = 96, 64, 4
    a = rng.integers(1, 256, (h, w), dtype=np.uint8)
    a[:16] = 16
    a[h - 24:] = 16
    a[:, :16] = 16
    a[:, w - 32:] = 16
    m = BS.plane_blockstat(a, k)
    assert BS.bars(m, w, h, k) == dict(top=1, bottom=1, left=1, right=2, level=16)
    f = BS.flat(m, w, h, k)
    assert f[0].all() and f[-1].all() and not f[1:3, 1:4].any()
    assert (BS.mean(m, w, h, k)[0] == 16).all() and (BS.variance(m, w, h, k)[0] == 0).all() and (BS.variance(m, w, h, k)[1, 1:4] > 0).all()
    b = a.copy()
    b[h - 24:] = 17  # the bottom bar at another level than the top one: no bar, and the side bars end in it
    assert BS.bars(BS.plane_blockstat(b, k), w, h, k) == dict(top=1, bottom=0, left=0, right=0, level=16)
    c = a.copy()
    c[5, 40] = 200  # one sample in the top bar
    assert BS.bars(BS.plane_blockstat(c, k), w, h, k)["top"] == 0
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    assert BS.bars(BS.plane_blockstat(noise, k), w, h, k) == dict(top=0, bottom=0, left=0, right=0, level=None)
    black = np.zeros((h, w), np.uint8)
    assert BS.bars(BS.plane_blockstat(black, 3), w, h, 3) == dict(top=8, bottom=0, left=0, right=0, level=0)
    # partial edge blocks: 100 x 70 at k = 5, a pillarbox of 32 columns left and the 4 columns of the last partial block right
    d = rng.integers(1, 256, (70, 100), dtype=np.uint8)
    d[:, :32] = 0
    d[:, 96:] = 0
    assert BS.bars(BS.plane_blockstat(d, 5), 100, 70, 5) == dict(top=0, bottom=0, left=1, right=1, level=0)
    with pytest.raises(ValueError):
        BS.flat(m, w + 16, h, k)


def test_blockstat_kernel_body_on_the_host_under_sanitizers(tmp_path):
    """tests/emu/blockstat_asan.cpp: blockstat_thread run over grids of 1 to 768 threads equals the plain definition for 12 widths x 12 heights x 4 strides x
    16 alignments x every k, the plane in a heap block that ends with its last byte and the map in a block of exactly its size -- the sanitizers see no access
    outside the two -- every record stored exactly once, and a 64 x 64 block of 255 and a checkerboard overflow nothing"""
    exe = str(tmp_path / "blockstat_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "blockstat_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])
    m = re.search(r"blockstat_asan: (\d+) cases, 0 wrong", r.stdout)
    assert m and int(m.group(1)) == 12 * 12 * 4 * 16 * 4 + 16, r.stdout[-500:]


def test_blockstat_kernel_resources(tmp_path):
    """e264_blockstat.hip cross-compiled for gfx950: the kernel spills nothing, uses no scratch, no AGPRs, no LDS and at most the VGPRs its header states
    (BS_VGPRS, itself at most 64: eight waves per SIMD)"""
    if not shutil.which(HIPCC):
        pytest.fail(f"no {HIPCC}: the cross-compiler is a tool of the build, not hardware")
    csrc = os.path.join(ROOT, "edge264_amd", "csrc")
    stated = re.search(r"^#define BS_VGPRS (\d+)", open(os.path.join(csrc, "e264_blockstat.h")).read(), re.M)
    assert stated and 0 < int(stated.group(1)) <= 64, "the header states the VGPR count (eight waves per SIMD: at most 64)"
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(csrc, "e264_blockstat.hip"), "-o", str(tmp_path / "b.o"),
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
    hits = {k: v for k, v in kernels.items() if "e264_blockstat_kernel" in k}
    assert len(hits) == 1, sorted(kernels)
    r = next(iter(hits.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, r
    assert 0 < r["VGPRs"] <= int(stated.group(1)) and r["AGPRs"] == 0, r


def test_library_surface_and_host_only_refusals():
    """the library loads without a GPU and has the entry points; e264hip_blockstat_bytes; e264hip_blockstat_check -- what e264hip_blockstat_batch runs for every
    picture before anything is queued -- refuses a block size outside 3..6 and a bad view, and names the cause; what the batch refuses before it looks at a
    device"""
    lib = backend.load_library()
    for name in ("e264hip_frame_blockstat", "e264hip_blockstat_batch", "e264hip_blockstat_check", "e264hip_blockstat_bytes"):
        assert hasattr(lib, name) and name in backend.EXPORTED_SYMBOLS
    v = D.frame_view(5, 3, crop=(2, 6, 2, 10))  # 72 x 36, chroma 36 x 18
    for k in KS:
        dims = [BS.blockstat_dims(w, h, k) for w, h in zip(v["width"], v["height"])]
        assert backend.blockstat_dims(v, k) == dims == backend.blockdiff_dims(v, k) and backend.blockstat_bytes(v, k) == 16 * sum(bw * bh for bw, bh in dims) == 2 * backend.blockdiff_bytes(v, k)
    assert backend.blockstat_dims(v, 3) == [(9, 5), (5, 3), (5, 3)] and backend.blockstat_dims(v, 6) == [(2, 1), (1, 1), (1, 1)]
    d = (C.c_uint16 * 6)(*[9] * 6)
    for k in (-1, 0, 2, 7, 64):
        assert lib.e264hip_blockstat_bytes(C.byref(backend.as_view(v)), k, d) == 0 and list(d) == [9] * 6
        with pytest.raises(ValueError):
            backend.blockstat_dims(v, k)
    assert backend.blockstat_bytes(None, 4) == 0
    empty = backend.as_view(v)
    empty.plane[2].width = 0
    assert backend.blockstat_bytes(empty, 4) == 0
    big = dict(offset=[0, 0, 0], stride=[65535] * 3, width=[65535] * 3, height=[65535] * 3)
    assert backend.blockstat_bytes(big, 3) == 3 * 8192 * 8192 * 16 and backend.blockstat_dims(big, 3) == [(8192, 8192)] * 3
    # the check: the view's refusals and the range of k
    geo = dict(stride_Y=96, stride_C=104, plane_size_Y=96 * 48, plane_size_C=104 * 24)
    va = D.frame_view(5, 3, crop=(2, 6, 2, 10), geometry=geo)
    na = 96 * 48 + 104 * 24
    for k in KS:
        assert backend.blockstat_check(va, na, k) == 0
    for k in (-1, 0, 1, 2, 7, 8, 1 << 20):
        assert backend.blockstat_check(va, na, k) == errno.EINVAL and "log2_block" in backend.last_error(), k
    assert lib.e264hip_blockstat_check(None, na, 4) == errno.EINVAL and "null" in backend.last_error()
    ea = max(o + (h - 1) * s + w for o, s, w, h in zip(va["offset"], va["stride"], va["width"], va["height"]))  # the view's last byte + 1
    assert ea <= na and backend.blockstat_check(va, ea, 4) == 0
    assert backend.blockstat_check(va, ea - 1, 4) == errno.EINVAL and "leaves the slot" in backend.last_error()
    for p in range(3):
        for field, text in (("width", "without samples"), ("height", "without samples"), ("stride", "stride below width")):
            bad = backend.as_view(va)
            setattr(bad.plane[p], field, 0)
            assert backend.blockstat_check(bad, na, 5) == errno.EINVAL and text in backend.last_error(), (p, field)
    # the batch, before it looks at a device: a null device, n < 0, n = 4097 -- EINVAL with a text, `out` untouched -- and the batch of one without a stream
    out = np.full(64, 7, np.uint8)
    for dev, n in ((None, 1), (None, -1), (None, 4097)):
        assert lib.e264hip_blockstat_batch(dev, None, None, None, n, 4, out.ctypes.data, 64) == errno.EINVAL and backend.last_error()
    assert lib.e264hip_frame_blockstat(None, 0, None, 4, out.ctypes.data, 64) == errno.EINVAL and "null stream" in backend.last_error()
    assert (out == 7).all()


def test_front_blockstat_library():
    """edge264_amd/libedge264_frontdigest.so exports e264front_frame_blockstat (edge264_amd/frontend/front_blockstat.c) beside the other passes' entry points,
    refuses null arguments, a view that is neither 0 nor 1 and a block size outside 3..6 before it looks for the front library or the back end, and answers
    ENODEV where the front library is not to be found"""
    path = os.path.join(ROOT, "edge264_amd", "libedge264_frontdigest.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    lib = C.CDLL(path)
    lib.e264front_frame_blockstat.restype = C.c_int
    lib.e264front_frame_blockstat.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.e264front_frame_digest, lib.e264front_frame_preview, lib.e264front_frame_diff, lib.e264front_frame_hist, lib.e264front_frame_blockdiff, lib.e264front_digest_use  # (still there)
    out = np.full(256, 7, np.uint8)
    dims = (C.c_uint16 * 6)(*[9] * 6)
    frame = (C.c_char * 128)()
    o = out.ctypes.data
    assert lib.e264front_frame_blockstat(None, frame, 0, 4, o, 256, dims) == errno.EINVAL
    assert lib.e264front_frame_blockstat(1, None, 0, 4, o, 256, dims) == errno.EINVAL
    assert lib.e264front_frame_blockstat(1, frame, 0, 4, None, 256, dims) == errno.EINVAL
    for view in (2, -1):
        assert lib.e264front_frame_blockstat(1, frame, view, 4, o, 256, dims) == errno.EINVAL
    for k in (-1, 0, 2, 7):
        assert lib.e264front_frame_blockstat(1, frame, 0, k, o, 256, dims) == errno.EINVAL
    assert (out == 7).all() and list(dims) == [9] * 6
    # without the front library: a copy of the library alone in a directory, in a process of its own (the binding is made once per process)
    code = ("import ctypes as C, shutil, sys, tempfile, os\n"
            "d = tempfile.mkdtemp()\n"
            "p = shutil.copy(sys.argv[1], os.path.join(d, 'libedge264_frontdigest.so'))\n"
            "os.environ.pop('E264_HIP_LIB', None)\n"
            "lib = C.CDLL(p)\n"
            "lib.e264front_frame_blockstat.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]\n"
            "f = (C.c_char * 128)(); o = (C.c_char * 96)()\n"
            "r = lib.e264front_frame_blockstat(1, f, 0, 4, o, 96, None)\n"
            "shutil.rmtree(d)\n"
            "print(r)\n")
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and int(r.stdout.strip()) == errno.ENODEV, (r.stdout, r.stderr[-2000:])
