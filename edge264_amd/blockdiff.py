"""The block difference map of include/edge264_hip.h (version 1) in numpy.

    k = 3 .. 6      b = 1 << k      bw = (w + b - 1) >> k      bh = (h + b - 1) >> k
    record (Y, X):  sad = sum |a - b|,  sse = sum (a - b)^2  over  y in [b Y, min(b Y + b, h)),  x in [b X, min(b X + b, w))

blockdiff_plane is what the device computes (backend.Stream.blockdiff, Device.blockdiff_batch; in C also e264front_frame_blockdiff) for two
planes the caller holds in host memory; include/edge264_blockdiff.h is the same in C.  A view is the dict digest.frame_view returns.
"""
from __future__ import annotations

import numpy as np

from .digest import view_planes

BLOCKDIFF_VERSION = 1
# E264BlockDiff as numpy sees it: a map is an array of shape (bh, bw) of this record (8 bytes)
BLOCKDIFF_DTYPE = np.dtype([("sad", "<u4"), ("sse", "<u4")])


def blockdiff_dims(w: int, h: int, k: int):
    """(bw, bh) of a plane of w x h samples at block size 1 << k"""
    if k not in (3, 4, 5, 6):
        raise ValueError("blockdiff: log2_block is none of 3, 4, 5, 6")
    if w < 1 or h < 1:
        raise ValueError("blockdiff: a plane without samples")
    b = 1 << k
    return (w + b - 1) >> k, (h + b - 1) >> k


def blockdiff_plane(a, b, k: int = 4) -> np.ndarray:
    """the map of two 2-D uint8 arrays of one shape (any strides: cropped views of slots are fine): a BLOCKDIFF_DTYPE array of shape (bh, bw)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("blockdiff_plane takes two 2-D uint8 arrays")
    if a.shape != b.shape:
        raise ValueError("blockdiff_plane: the two planes differ in size")
    h, w = a.shape
    bw, bh = blockdiff_dims(w, h, k)
    d = np.zeros((bh << k, bw << k), np.int64)  # samples outside the plane: no difference
    d[:h, :w] = np.abs(a.astype(np.int64) - b.astype(np.int64))
    d = d.reshape(bh, 1 << k, bw, 1 << k)
    out = np.zeros((bh, bw), BLOCKDIFF_DTYPE)
    out["sad"] = d.sum(axis=(1, 3))
    out["sse"] = (d * d).sum(axis=(1, 3))
    return out


def frame_blockdiff(view_a: dict, img_a: np.ndarray, view_b: dict, img_b: np.ndarray, k: int = 4):
    """[Y, Cb, Cr] maps of two slots' host copies"""
    return [blockdiff_plane(p, q, k) for p, q in zip(view_planes(view_a, img_a), view_planes(view_b, img_b))]


def changed(m) -> np.ndarray:
    """the boolean mask of a map: True where the block's samples differ (sad != 0, which is sse != 0)"""
    return np.asarray(m)["sad"] != 0


def psnr_map(m, w: int, h: int, k: int) -> np.ndarray:
    """10 log10(255^2 n / sse) per block of the map of a plane of w x h samples, n the samples the block has inside the plane; inf where sse == 0"""
    m = np.asarray(m)
    bw, bh = blockdiff_dims(w, h, k)
    if m.shape != (bh, bw):
        raise ValueError("psnr_map: the map is not this plane's")
    b = 1 << k
    rows = np.minimum(b, h - b * np.arange(bh)).astype(np.float64)
    cols = np.minimum(b, w - b * np.arange(bw)).astype(np.float64)
    n = rows[:, None] * cols[None, :]
    sse = m["sse"].astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 * 255.0 * n / np.where(sse == 0, 1.0, sse)))


def split_map(buf: np.ndarray, dims):
    """one pair's map bytes (Y | Cb | Cr) as three 2-D BLOCKDIFF_DTYPE arrays; dims: [(bw, bh)] * 3"""
    out, at = [], 0
    for bw, bh in dims:
        n = bw * bh * BLOCKDIFF_DTYPE.itemsize
        out.append(np.frombuffer(bytes(buf[at:at + n]), BLOCKDIFF_DTYPE).reshape(bh, bw).copy())
        at += n
    return out
