"""The histogram record of include/edge264_hip.h (version 1) in numpy, and the arithmetic on its bins.

    bin[p][v] = the number of samples of plane p equal to v, v in 0..255

hist_plane is what the device computes (backend.Stream.hist, Device.hist_batch; in C also e264front_frame_hist) for a plane the caller
holds in host memory; include/edge264_hist.h is the same in C.  stats, quantile and distance are what the device leaves to the host:
arithmetic on 256 numbers.  A view is the dict digest.frame_view returns.
"""
from __future__ import annotations

import numpy as np

from .digest import view_planes

HIST_VERSION = 1


def hist_plane(plane) -> np.ndarray:
    """the 256 bins (uint32) of a 2-D uint8 array (any strides: a cropped view of a slot is fine)"""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("hist_plane takes a 2-D uint8 array")
    return np.bincount(np.ascontiguousarray(a).reshape(-1), minlength=256).astype(np.uint32)


def frame_hist(view: dict, img: np.ndarray) -> np.ndarray:
    """the (3, 256) record of a slot's host copy: Y, Cb, Cr"""
    return np.stack([hist_plane(p) for p in view_planes(view, img)])


def _bins(bins) -> np.ndarray:
    b = np.asarray(bins)
    if b.shape != (256,):
        raise ValueError("one plane's 256 bins")
    return b.astype(np.uint64)


def stats(bins) -> dict:
    """count, min, max, sum, sum2 of one plane's bins (ints; min = 255 and max = 0 for an empty histogram): mean = sum / count,
    variance = sum2 / count - mean ** 2"""
    b = _bins(bins)
    v = np.arange(256, dtype=np.uint64)
    nz = np.flatnonzero(b)
    return dict(count=int(b.sum()), min=int(nz[0]) if nz.size else 255, max=int(nz[-1]) if nz.size else 0, sum=int((v * b).sum()), sum2=int((v * v * b).sum()))


def quantile(bins, num: int, den: int) -> int:
    """the smallest v with at least num / den of the samples at or below it: (bin[0] + .. + bin[v]) * den >= count * num (e264_hist_quantile);
    0 for num = 0 and for an empty histogram, the largest occupied v for num = den"""
    below = [int(x) for x in np.cumsum(_bins(bins))]
    for v in range(255):
        if below[v] * den >= below[255] * num:
            return v
    return 255


def distance(a, b) -> int:
    """the L1 distance of two planes' bins, sum |a[v] - b[v]|: the scene-cut measure (0 .. the two counts' sum)"""
    return int(np.abs(_bins(a).astype(np.int64) - _bins(b).astype(np.int64)).sum())
