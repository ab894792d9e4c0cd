"""The picture digest of include/edge264_hip.h (version 1) in numpy, and the view of a picture in a slot.

    fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16      (mod 2^32)
    K(i) = fmix32(i) | 1
    D    = sum over i = y * w + x of (s[y][x] + 1) * K(i)                                       (mod 2^64)

plane_digest is what the device computes (backend.Stream.digest, Device.digest_batch; in C also e264front_frame_digest) for a plane the
caller holds in host memory; include/edge264_digest.h is the same in C.  Not cryptographic.
"""
from __future__ import annotations

import numpy as np

from . import packet as P

DIGEST_VERSION = 1
_CHUNK = 1 << 20  # samples per step: the weights are made on the fly, 4 MB at a time


def fmix32(i: np.ndarray) -> np.ndarray:
    h = np.asarray(i, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return h


def plane_digest(plane) -> int:
    """D of a 2-D array of samples (any strides: a cropped view of a slot is fine)."""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("plane_digest takes a 2-D uint8 array")
    s = np.ascontiguousarray(a).reshape(-1)
    d = 0
    with np.errstate(over="ignore"):
        for lo in range(0, s.size, _CHUNK):
            part = s[lo:lo + _CHUNK]
            k = (fmix32(np.arange(lo, lo + part.size, dtype=np.uint32)) | np.uint32(1)).astype(np.uint64)
            d += int(((part.astype(np.uint64) + np.uint64(1)) * k).sum(dtype=np.uint64))  # (products below 2^41; the sum wraps as the definition does)
    return d & 0xffffffffffffffff


def frame_view(width_mbs: int, height_mbs: int, crop=(0, 0, 0, 0), geometry=None) -> dict:
    """Where the picture of width_mbs x height_mbs macroblocks, cropped by crop = (left, right, top, bottom) luma samples (even numbers: 4:2:0),
    lies in a slot: {"offset": [Y, Cb, Cr], "stride": [...], "width": [...], "height": [...]} -- the fields of E264View.  geometry: the four
    layout fields of a packet header (stride_Y, stride_C, plane_size_Y, plane_size_C); default packet.frame_geometry, the reference's layout."""
    g = geometry if geometry is not None else P.frame_geometry(width_mbs, height_mbs)
    l, r, t, b = (int(x) for x in crop)
    if min(l, r, t, b) < 0 or (l | r | t | b) & 1:
        raise ValueError("crop: four even numbers >= 0")
    w, h = width_mbs * 16 - l - r, height_mbs * 16 - t - b
    if w < 2 or h < 2:
        raise ValueError("crop leaves no picture")
    sy, sc, psy = int(g["stride_Y"]), int(g["stride_C"]), int(g["plane_size_Y"])
    cb = psy + (t >> 1) * sc + (l >> 1)
    return dict(offset=[t * sy + l, cb, cb + (sc >> 1)], stride=[sy, sc, sc], width=[w, w >> 1, w >> 1], height=[h, h >> 1, h >> 1])


def view_planes(view: dict, slot: np.ndarray):
    """the three planes a view names, as 2-D views of a slot's bytes (what plane_digest takes)"""
    out = []
    for o, s, w, h in zip(view["offset"], view["stride"], view["width"], view["height"]):
        out.append(np.lib.stride_tricks.as_strided(slot[o:], shape=(h, w), strides=(s, 1), writeable=False))
    return out


def frame_digest(view: dict, slot: np.ndarray):
    """(Y, Cb, Cr) digests of a slot's host copy"""
    return tuple(plane_digest(p) for p in view_planes(view, slot))
