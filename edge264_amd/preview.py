"""The reduced preview of include/edge264_hip.h (version 1) in numpy.

    k = 1, 2, 3      f = 1 << k      ow = (w + f - 1) >> k      oh = (h + f - 1) >> k
    P[Y][X] = (sum over dy < f, dx < f of s[min(f Y + dy, h - 1)][min(f X + dx, w - 1)]  +  (1 << (2 k - 1))) >> 2 k

plane_preview is what the device computes (backend.Stream.preview, Device.preview_batch; in C also e264front_frame_preview) for a plane the
caller holds in host memory; include/edge264_preview.h is the same in C.  A view is the dict digest.frame_view returns.
"""
from __future__ import annotations

import numpy as np

from .digest import view_planes

PREVIEW_VERSION = 1


def preview_dims(w: int, h: int, k: int):
    """(ow, oh) of a plane of w x h samples"""
    if k not in (1, 2, 3) or w < 1 or h < 1:
        raise ValueError("preview: k is 1, 2 or 3 and the plane has samples")
    f = 1 << k
    return (w + f - 1) >> k, (h + f - 1) >> k


def plane_preview(plane, k: int) -> np.ndarray:
    """P of a 2-D array of samples (any strides: a cropped view of a slot is fine): a new (oh, ow) uint8 array."""
    a = np.asarray(plane)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("plane_preview takes a 2-D uint8 array")
    h, w = a.shape
    ow, oh = preview_dims(w, h, k)
    f = 1 << k
    # a box that leaves the plane repeats its last column or row
    padded = np.pad(a, ((0, oh * f - h), (0, ow * f - w)), mode="edge").astype(np.uint32)
    sums = padded.reshape(oh, f, ow, f).sum(axis=(1, 3), dtype=np.uint32)
    return ((sums + (1 << (2 * k - 1))) >> (2 * k)).astype(np.uint8)


def frame_preview(view: dict, slot: np.ndarray, k: int):
    """[Y, Cb, Cr] previews of a slot's host copy"""
    return [plane_preview(p, k) for p in view_planes(view, slot)]


def preview_bytes(view: dict, k: int) -> int:
    """bytes of one picture's preview (Y | Cb | Cr, each plane tight)"""
    return sum(ow * oh for ow, oh in (preview_dims(w, h, k) for w, h in zip(view["width"], view["height"])))
