"""The difference record of include/edge264_hip.h (version 1) in numpy.

    i = y * w + x      d_i = |a_i - b_i|
    sad = sum d_i    sse = sum d_i^2    count = #{i: d_i != 0}    max = max d_i    first = min {i: d_i != 0} or DIFF_NONE

diff_plane is what the device computes (backend.Stream.diff, Device.diff_batch; in C also e264front_frame_diff) for two planes the
caller holds in host memory; include/edge264_diff.h is the same in C.  A view is the dict digest.frame_view returns.
"""
from __future__ import annotations

import math

import numpy as np

from .digest import view_planes

DIFF_VERSION = 1
DIFF_NONE = 0xffffffff
FIELDS = ("sad", "sse", "count", "first", "max")


def diff_plane(a, b) -> dict:
    """the record of two 2-D uint8 arrays of one shape (any strides: cropped views of slots are fine): a dict of five ints"""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("diff_plane takes two 2-D uint8 arrays")
    if a.shape != b.shape:
        raise ValueError("diff_plane: the two planes differ in size")
    d = np.abs(a.astype(np.int32) - b.astype(np.int32)).reshape(-1).astype(np.uint64)
    nz = np.flatnonzero(d)
    return dict(sad=int(d.sum(dtype=np.uint64)), sse=int((d * d).sum(dtype=np.uint64)), count=int(nz.size),
                first=int(nz[0]) if nz.size else DIFF_NONE, max=int(d.max()) if d.size else 0)


def frame_diff(view_a: dict, img_a: np.ndarray, view_b: dict, img_b: np.ndarray):
    """[Y, Cb, Cr] records of two slots' host copies"""
    return [diff_plane(p, q) for p, q in zip(view_planes(view_a, img_a), view_planes(view_b, img_b))]


def psnr(sse: int, w: int, h: int) -> float:
    """10 log10(255^2 w h / sse) of a plane of w x h samples; inf for sse == 0"""
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 * 255.0 * w * h / sse)


def as_dicts(rec) -> list:
    """one picture's device record (a backend.DIFF_DTYPE array of shape (3,)) as frame_diff gives it"""
    return [{f: int(rec[p][f]) for f in FIELDS} for p in range(3)]
