"""The block statistics map of include/edge264_hip.h (version 1) in numpy, and the arithmetic on its records.

    k = 3 .. 6      b = 1 << k      bw = (w + b - 1) >> k      bh = (h + b - 1) >> k
    record (Y, X), over the samples s(y, x) with  y in [b Y, min(b Y + b, h)),  x in [b X, min(b X + b, w)):
        sum = sum s      sumsq = sum s^2
        gh = sum |s(y, x + 1) - s(y, x)|  over those with x + 1 < w      gv = sum |s(y + 1, x) - s(y, x)|  over those with y + 1 < h

A pair belongs to the block of its left (gh) or top (gv) sample; a pair that would leave the plane does not exist.  plane_blockstat is what the
device computes (backend.Stream.blockstat, Device.blockstat_batch; in C also e264front_frame_blockstat) for a plane the caller holds in host
memory; include/edge264_blockstat.h is the same in C.  counts, mean, variance, flat and bars are what the device leaves to the host: arithmetic
on the records.  A view is the dict digest.frame_view returns.
"""
from __future__ import annotations

import numpy as np

from .digest import view_planes

BLOCKSTAT_VERSION = 1
# E264BlockStat as numpy sees it: a map is an array of shape (bh, bw) of this record (16 bytes)
BLOCKSTAT_DTYPE = np.dtype([("sum", "<u4"), ("sumsq", "<u4"), ("gh", "<u4"), ("gv", "<u4")])


def blockstat_dims(w: int, h: int, k: int):
    """(bw, bh) of a plane of w x h samples at block size 1 << k"""
    if k not in (3, 4, 5, 6):
        raise ValueError("blockstat: log2_block is none of 3, 4, 5, 6")
    if w < 1 or h < 1:
        raise ValueError("blockstat: a plane without samples")
    b = 1 << k
    return (w + b - 1) >> k, (h + b - 1) >> k


def _block_sums(a: np.ndarray, bw: int, bh: int, k: int) -> np.ndarray:
    """a (h' x w', int64, h' <= bh << k, w' <= bw << k) summed over blocks of 1 << k: what lies outside a adds nothing"""
    d = np.zeros((bh << k, bw << k), np.int64)
    d[:a.shape[0], :a.shape[1]] = a
    return d.reshape(bh, 1 << k, bw, 1 << k).sum(axis=(1, 3))


def plane_blockstat(plane, k: int = 4) -> np.ndarray:
    """the map of a 2-D uint8 array (any strides: a cropped view of a slot is fine): a BLOCKSTAT_DTYPE array of shape (bh, bw)"""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("plane_blockstat takes a 2-D uint8 array")
    h, w = a.shape
    bw, bh = blockstat_dims(w, h, k)
    s = a.astype(np.int64)
    out = np.zeros((bh, bw), BLOCKSTAT_DTYPE)
    out["sum"] = _block_sums(s, bw, bh, k)
    out["sumsq"] = _block_sums(s * s, bw, bh, k)
    out["gh"] = _block_sums(np.abs(s[:, 1:] - s[:, :-1]), bw, bh, k)  # pair (y, x), (y, x + 1) at (y, x): its left sample's block; column w - 1 has none
    out["gv"] = _block_sums(np.abs(s[1:, :] - s[:-1, :]), bw, bh, k)  # pair (y, x), (y + 1, x) at (y, x): its top sample's block; row h - 1 has none
    return out


def frame_blockstat(view: dict, img: np.ndarray, k: int = 4):
    """[Y, Cb, Cr] maps of a slot's host copy"""
    return [plane_blockstat(p, k) for p in view_planes(view, img)]


def counts(w: int, h: int, k: int) -> np.ndarray:
    """the samples per block of the map of a plane of w x h samples: an int64 array of shape (bh, bw)"""
    bw, bh = blockstat_dims(w, h, k)
    b = 1 << k
    rows = np.minimum(b, h - b * np.arange(bh)).astype(np.int64)
    cols = np.minimum(b, w - b * np.arange(bw)).astype(np.int64)
    return rows[:, None] * cols[None, :]


def _counts_of(m: np.ndarray, w: int, h: int, k: int) -> np.ndarray:
    n = counts(w, h, k)
    if np.asarray(m).shape != n.shape:
        raise ValueError("blockstat: the map is not this plane's")
    return n


def mean(m, w: int, h: int, k: int) -> np.ndarray:
    """sum / n per block (float64)"""
    n = _counts_of(m, w, h, k)
    return np.asarray(m)["sum"].astype(np.float64) / n


def variance(m, w: int, h: int, k: int) -> np.ndarray:
    """(n sumsq - sum^2) / n^2 per block (float64; the numerator exact in 64-bit integers)"""
    n = _counts_of(m, w, h, k)
    m = np.asarray(m)
    s = m["sum"].astype(np.int64)
    return (n * m["sumsq"].astype(np.int64) - s * s).astype(np.float64) / (n * n).astype(np.float64)


def flat(m, w: int, h: int, k: int) -> np.ndarray:
    """the boolean mask of a map: True where every sample of the block has one value, n sumsq == sum^2 in 64-bit integers"""
    n = _counts_of(m, w, h, k)
    m = np.asarray(m)
    s = m["sum"].astype(np.int64)
    return n * m["sumsq"].astype(np.int64) == s * s


def bars(map_y, w: int, h: int, k: int) -> dict:
    """Letterbox and pillarbox bars of a luma map of a plane of w x h samples: the leading and trailing block rows and columns whose blocks are all
    flat AT ONE LEVEL (every block of the run has the level of the run's first block): dict(top, bottom, left, right) in blocks, and level, the
    bars' sample value (None without bars).  Rows are counted first; columns are counted over the block rows between the bars.  A picture that is
    flat throughout is all `top`."""
    n = _counts_of(map_y, w, h, k)
    m = np.asarray(map_y)
    f = flat(m, w, h, k)
    lvl = m["sum"].astype(np.int64) // n  # a flat block's level
    bh, bw = f.shape

    def run(ok_of, length):
        c = 0
        while c < length and ok_of(c):
            c += 1
        return c

    level = [None]

    def line_ok(fl, lv):
        if not fl.all():
            return False
        if level[0] is None:
            if not (lv == lv.flat[0]).all():
                return False
            level[0] = int(lv.flat[0])
            return True
        return bool((lv == level[0]).all())

    top = run(lambda y: line_ok(f[y], lvl[y]), bh)
    bottom = run(lambda y: line_ok(f[bh - 1 - y], lvl[bh - 1 - y]), bh - top)
    mid = slice(top, bh - bottom)
    left = right = 0
    if top < bh:
        left = run(lambda x: line_ok(f[mid, x], lvl[mid, x]), bw)
        right = run(lambda x: line_ok(f[mid, bw - 1 - x], lvl[mid, bw - 1 - x]), bw - left)
    return dict(top=top, bottom=bottom, left=left, right=right, level=level[0] if top or bottom or left or right else None)


def split_map(buf: np.ndarray, dims):
    """one picture's map bytes (Y | Cb | Cr) as three 2-D BLOCKSTAT_DTYPE arrays; dims: [(bw, bh)] * 3"""
    out, at = [], 0
    for bw, bh in dims:
        n = bw * bh * BLOCKSTAT_DTYPE.itemsize
        out.append(np.frombuffer(bytes(buf[at:at + n]), BLOCKSTAT_DTYPE).reshape(bh, bw).copy())
        at += n
    return out
