"""ctypes binding of the C-ABI back end (include/edge264_hip.h, libedge264_hip.so).

This is plumbing around the product, not the product: the reconstruction itself is the
hand-written gfx950 HIP code in edge264_amd/csrc.  There is NO CPU fallback here: if the
shared library is missing or no MI355X is present, opening a device raises.
"""
from __future__ import annotations

import ctypes as C
import errno
import os

import numpy as np

from . import packet as P
from .blockstat import BLOCKSTAT_DTYPE, split_map as _split_blockstat  # E264BlockStat as numpy sees it (16 bytes) and a map's bytes as three 2-D arrays of it

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E264_HIP_LIB") or os.path.join(HERE, "libedge264_hip.so")  # E264_HIP_LIB: A/B builds (csrc/Makefile `variant`)
RUN_RECON, RUN_DEBLOCK, RUN_ALL = 1, 2, 3
MAX_LANES = 4

_lib = None


class BackendError(RuntimeError):
    pass


class PlaneView(C.Structure):  # E264PlaneView of include/edge264_hip.h
    _fields_ = [("offset", C.c_uint32), ("stride", C.c_uint32), ("width", C.c_uint16), ("height", C.c_uint16)]


class View(C.Structure):  # E264View: Y, Cb, Cr
    _fields_ = [("plane", PlaneView * 3)]


DIGEST_MAX_BATCH = 4096
PREVIEW_MAX_BATCH = 4096
PREVIEW_MAX_BYTES = 1 << 28
DIFF_MAX_BATCH = 4096
DIFF_NONE = 0xffffffff
# E264Diff as numpy sees it: an array of shape (n, 3) -- pictures, then Y, Cb, Cr -- of this record (E264PlaneDiff, 32 bytes)
DIFF_DTYPE = np.dtype([("sad", "<u8"), ("sse", "<u8"), ("count", "<u4"), ("first", "<u4"), ("max", "<u4"), ("zero", "<u4")])
BLOCKDIFF_MAX_BATCH = 4096
BLOCKDIFF_MAX_BYTES = 1 << 28
# E264BlockDiff as numpy sees it: a plane's map is an array of shape (bh, bw) of this record (8 bytes)
BLOCKDIFF_DTYPE = np.dtype([("sad", "<u4"), ("sse", "<u4")])
BLOCKSTAT_MAX_BATCH = 4096
BLOCKSTAT_MAX_BYTES = 1 << 28
HIST_MAX_BATCH = 4096  # E264Hist as numpy sees it: uint32 of shape (n, 3, 256) -- pictures, then Y, Cb, Cr, then the sample value


def as_view(view) -> View:
    """a View, or the dict digest.frame_view returns ({"offset": [Y, Cb, Cr], "stride": ..., "width": ..., "height": ...}), as the C structure"""
    if isinstance(view, View):
        return view
    v = View()
    for p in range(3):
        v.plane[p] = PlaneView(int(view["offset"][p]), int(view["stride"][p]), int(view["width"][p]), int(view["height"][p]))
    return v


def load_library():
    """Loads libedge264_hip.so (in-tree, built by __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP back end has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    sig = {
        "e264hip_device_open": (i, [i, C.POINTER(vp)]),
        "e264hip_device_close": (None, [vp]),
        "e264hip_device_sync": (i, [vp]),
        "e264hip_last_error": (C.c_char_p, []),
        "e264hip_stream_open": (i, [vp, C.POINTER(vp)]),
        "e264hip_stream_close": (None, [vp]),
        "e264hip_stream_bind_lane": (i, [vp, i]),
        "e264hip_stream_flush": (i, [vp]),
        "e264hip_frame_alloc": (i, [vp, i, sz, C.POINTER(vp)]),
        "e264hip_frame_free": (None, [vp, i]),
        "e264hip_frame_fill": (i, [vp, i, i]),
        "e264hip_frame_upload": (i, [vp, i, vp, sz]),
        "e264hip_frame_submit": (i, [vp, vp, sz]),
        "e264hip_packet_buffer": (vp, [vp, sz]),
        "e264hip_frame_wait": (i, [vp, i]),
        "e264hip_frame_download": (i, [vp, i, vp, sz]),
        "e264hip_packet_upload": (i, [vp, vp, sz, C.POINTER(vp)]),
        "e264hip_packet_free": (None, [vp]),
        "e264hip_submit_batch": (i, [vp, C.POINTER(vp), C.POINTER(vp), i, i]),
        "e264hip_packet_check": (i, [vp, sz]),
        "e264hip_packet_compact_bound": (sz, [vp, sz]),
        "e264hip_packet_compact": (sz, [vp, sz, vp, sz]),
        "e264hip_packet_compact2_bound": (sz, [vp, sz, i]),
        "e264hip_packet_compact2": (sz, [vp, sz, i, vp, sz]),
        "e264hip_packet_fold_bound": (sz, [vp, sz, i]),
        "e264hip_packet_fold": (sz, [vp, sz, i, vp, sz]),
        "e264hip_packet_expand": (sz, [vp, sz, vp, sz]),
        "e264hip_submit_batch_host": (i, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), i, i]),
        "e264hip_submit_batch_pinned": (i, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), i, i, i]),
        "e264hip_host_alloc": (vp, [vp, sz]),
        "e264hip_host_free": (None, [vp, vp]),
        "e264hip_batch_create": (i, [vp, C.POINTER(vp), C.POINTER(vp), i, C.POINTER(vp)]),
        "e264hip_batch_submit": (i, [vp, i]),
        "e264hip_batch_free": (None, [vp]),
        "e264hip_event_record": (i, [vp, i]),
        "e264hip_event_elapsed_ms": (i, [vp, i, i, C.POINTER(C.c_float)]),
        "e264hip_event_query": (i, [vp, i]),
        "e264hip_kernel_timing": (i, [vp, i]),
        "e264hip_kernel_time_ms": (i, [vp, C.POINTER(C.c_double), C.POINTER(i)]),
        "e264hip_set_option": (i, [vp, C.c_char_p, i]),
        "e264hip_build_flags": (C.c_char_p, []),
        "e264hip_frame_device_ptr": (vp, [vp, i]),
        "e264hip_launch_counts": (i, [vp, C.POINTER(C.c_uint64), i, i]),
        "e264hip_view_check": (i, [C.POINTER(View), sz]),
        "e264hip_frame_digest": (i, [vp, i, C.POINTER(View), C.POINTER(C.c_uint64)]),
        "e264hip_digest_batch": (i, [vp, C.POINTER(vp), C.POINTER(i), C.POINTER(View), i, C.POINTER(C.c_uint64)]),
        "e264hip_preview_bytes": (sz, [C.POINTER(View), i, C.POINTER(C.c_uint16)]),
        "e264hip_frame_preview": (i, [vp, i, C.POINTER(View), i, vp, sz]),
        "e264hip_preview_batch": (i, [vp, C.POINTER(vp), C.POINTER(i), C.POINTER(View), i, i, vp, sz]),
        "e264hip_diff_check": (i, [C.POINTER(View), sz, C.POINTER(View), sz]),
        "e264hip_frame_diff": (i, [vp, i, C.POINTER(View), vp, i, C.POINTER(View), vp]),
        "e264hip_diff_batch": (i, [vp, C.POINTER(vp), C.POINTER(i), C.POINTER(View), C.POINTER(vp), C.POINTER(i), C.POINTER(View), i, vp]),
        "e264hip_frame_hist": (i, [vp, i, C.POINTER(View), vp]),
        "e264hip_hist_batch": (i, [vp, C.POINTER(vp), C.POINTER(i), C.POINTER(View), i, vp]),
        "e264hip_blockdiff_bytes": (sz, [C.POINTER(View), i, C.POINTER(C.c_uint16)]),
        "e264hip_blockdiff_check": (i, [C.POINTER(View), sz, C.POINTER(View), sz, i]),
        "e264hip_frame_blockdiff": (i, [vp, i, C.POINTER(View), vp, i, C.POINTER(View), i, vp, sz]),
        "e264hip_blockdiff_batch": (i, [vp, C.POINTER(vp), C.POINTER(i), C.POINTER(View), C.POINTER(vp), C.POINTER(i), C.POINTER(View), i, i, vp, sz]),
        "e264hip_blockstat_bytes": (sz, [C.POINTER(View), i, C.POINTER(C.c_uint16)]),
        "e264hip_blockstat_check": (i, [C.POINTER(View), sz, i]),
        "e264hip_frame_blockstat": (i, [vp, i, C.POINTER(View), i, vp, sz]),
        "e264hip_blockstat_batch": (i, [vp, C.POINTER(vp), C.POINTER(i), C.POINTER(View), i, i, vp, sz]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the library does not export the header's symbol
        fn.restype, fn.argtypes = res, args
    flags = (L.e264hip_build_flags() or b"").decode()
    if ("E264_ABL_" in flags or "E264_PHASE_" in flags) and os.environ.get("E264_ALLOW_ABLATION") != "1":
        raise BackendError(f"{LIB_PATH} is a timing-ablation build ({flags.strip()}): its samples are wrong by design; "
                           "set E264_ALLOW_ABLATION=1 to load it (tools/visits/gpu_ab.sh does)")
    _lib = L
    return L


def build_flags() -> str:
    """Build-time switches of the loaded library ("" = product build)."""
    return (load_library().e264hip_build_flags() or b"").decode().strip()


EXPORTED_SYMBOLS = [
    "e264hip_device_open", "e264hip_device_close", "e264hip_device_sync", "e264hip_last_error",
    "e264hip_stream_open", "e264hip_stream_close", "e264hip_stream_bind_lane", "e264hip_stream_flush", "e264hip_frame_alloc",
    "e264hip_frame_free", "e264hip_frame_fill", "e264hip_frame_upload", "e264hip_frame_submit",
    "e264hip_packet_buffer", "e264hip_frame_wait", "e264hip_frame_download", "e264hip_packet_upload",
    "e264hip_packet_free", "e264hip_packet_check", "e264hip_packet_compact_bound", "e264hip_packet_compact", "e264hip_packet_compact2_bound", "e264hip_packet_compact2", "e264hip_packet_fold_bound", "e264hip_packet_fold", "e264hip_packet_expand", "e264hip_submit_batch", "e264hip_submit_batch_host", "e264hip_submit_batch_pinned", "e264hip_host_alloc", "e264hip_host_free", "e264hip_batch_create", "e264hip_batch_submit", "e264hip_batch_free", "e264hip_event_record", "e264hip_event_elapsed_ms", "e264hip_event_query",
    "e264hip_kernel_timing", "e264hip_kernel_time_ms", "e264hip_set_option", "e264hip_build_flags", "e264hip_frame_device_ptr",
    "e264hip_launch_counts", "e264hip_view_check", "e264hip_frame_digest", "e264hip_digest_batch",
    "e264hip_preview_bytes", "e264hip_frame_preview", "e264hip_preview_batch",
    "e264hip_diff_check", "e264hip_frame_diff", "e264hip_diff_batch",
    "e264hip_frame_hist", "e264hip_hist_batch",
    "e264hip_blockdiff_bytes", "e264hip_blockdiff_check", "e264hip_frame_blockdiff", "e264hip_blockdiff_batch",
    "e264hip_blockstat_bytes", "e264hip_blockstat_check", "e264hip_frame_blockstat", "e264hip_blockstat_batch",
]

# slots of e264hip_launch_counts (E264_LC_NAMES in include/edge264_hip.h): "n_cus" is the device's compute-unit count, every
# other slot the pictures that went through one kernel form
LAUNCH_COUNT_NAMES = ("n_cus expand dbkp_small dbkp_general dbkp_side1 dbkp_side2 pred "
                      "intra4_bitmap intra8_bitmap intra16_bitmap intra4_nobitmap intra8_nobitmap intra16_nobitmap "
                      "intra_split intra_planes_split intra_planes_alone dbk_planes dbk2_6 dbk2_7 dbk2_8 dbk2_10 dbk2_12 dbk_2 dbk_4 dbk_7 dbk_8").split()


def _check(L, r: int, what: str) -> None:
    if r:
        msg = L.e264hip_last_error()
        raise BackendError(f"{what}: {errno.errorcode.get(r, r)} ({(msg or b'').decode()})")


def preview_dims(view, k: int):
    """[(ow, oh)] of Y, Cb, Cr of a view's preview at reduction k, from the library (host only); raises for what has none"""
    d = (C.c_uint16 * 6)()
    if not load_library().e264hip_preview_bytes(C.byref(as_view(view)), k, d):
        raise ValueError("preview: k is 1, 2 or 3 and every plane of the view has samples")
    return [(int(d[2 * p]), int(d[2 * p + 1])) for p in range(3)]


def preview_bytes(view, k: int) -> int:
    """e264hip_preview_bytes: the bytes of a view's preview at reduction k (Y | Cb | Cr, each plane tight); 0 for what has none.  Host only."""
    return int(load_library().e264hip_preview_bytes(C.byref(as_view(view)) if view is not None else None, k, None))


def diff_check(view_a, slot_bytes_a: int, view_b, slot_bytes_b: int) -> int:
    """e264hip_diff_check: 0, or EINVAL (last_error() names the cause) for a pair of views a difference record cannot be made of.  Host only."""
    return int(load_library().e264hip_diff_check(C.byref(as_view(view_a)), slot_bytes_a, C.byref(as_view(view_b)), slot_bytes_b))


def blockdiff_dims(view, k: int):
    """[(bw, bh)] of Y, Cb, Cr of a view's block difference map at block size 1 << k, from the library (host only); raises for what has none"""
    d = (C.c_uint16 * 6)()
    if not load_library().e264hip_blockdiff_bytes(C.byref(as_view(view)), k, d):
        raise ValueError("blockdiff: k is 3, 4, 5 or 6 and every plane of the view has samples")
    return [(int(d[2 * p]), int(d[2 * p + 1])) for p in range(3)]


def blockdiff_bytes(view, k: int) -> int:
    """e264hip_blockdiff_bytes: the bytes of a view's block difference map at block size 1 << k (Y | Cb | Cr, each plane tight); 0 for what has none.  Host only."""
    return int(load_library().e264hip_blockdiff_bytes(C.byref(as_view(view)) if view is not None else None, k, None))


def blockdiff_check(view_a, slot_bytes_a: int, view_b, slot_bytes_b: int, k: int) -> int:
    """e264hip_blockdiff_check: 0, or EINVAL (last_error() names the cause) for a pair of views or a block size a map cannot be made of.  Host only."""
    return int(load_library().e264hip_blockdiff_check(C.byref(as_view(view_a)), slot_bytes_a, C.byref(as_view(view_b)), slot_bytes_b, k))


def _split_blockdiff(buf: np.ndarray, dims):
    out, at = [], 0
    for bw, bh in dims:
        n = bw * bh * BLOCKDIFF_DTYPE.itemsize
        out.append(buf[at:at + n].view(BLOCKDIFF_DTYPE).reshape(bh, bw))
        at += n
    return out


def blockstat_dims(view, k: int):
    """[(bw, bh)] of Y, Cb, Cr of a view's block statistics map at block size 1 << k, from the library (host only); raises for what has none"""
    d = (C.c_uint16 * 6)()
    if not load_library().e264hip_blockstat_bytes(C.byref(as_view(view)), k, d):
        raise ValueError("blockstat: k is 3, 4, 5 or 6 and every plane of the view has samples")
    return [(int(d[2 * p]), int(d[2 * p + 1])) for p in range(3)]


def blockstat_bytes(view, k: int) -> int:
    """e264hip_blockstat_bytes: the bytes of a view's block statistics map at block size 1 << k (Y | Cb | Cr, each plane tight); 0 for what has none.  Host only."""
    return int(load_library().e264hip_blockstat_bytes(C.byref(as_view(view)) if view is not None else None, k, None))


def blockstat_check(view, slot_bytes: int, k: int) -> int:
    """e264hip_blockstat_check: 0, or EINVAL (last_error() names the cause) for a view or a block size a map cannot be made of.  Host only."""
    return int(load_library().e264hip_blockstat_check(C.byref(as_view(view)), slot_bytes, k))


def _split_preview(buf: np.ndarray, dims):
    out, at = [], 0
    for ow, oh in dims:
        out.append(buf[at:at + ow * oh].reshape(oh, ow))
        at += ow * oh
    return out


def packet_check(pkt: bytes) -> int:
    """Host-only validation (no GPU needed): 0 or an errno value."""
    L = load_library()
    buf = (C.c_char * len(pkt)).from_buffer_copy(pkt)
    return L.e264hip_packet_check(C.cast(buf, C.c_void_p), len(pkt))


def packet_compact(pkt: bytes, level: int = 1) -> bytes:
    """A version-4 packet in its WIRE form (include/edge264_compact.h): level 1 gives version 5, level 2 version 6 (macroblocks of one partition
    with residual folded too).  Host only."""
    L = load_library()
    src = (C.c_char * len(pkt)).from_buffer_copy(pkt)
    cap = L.e264hip_packet_compact2_bound(C.cast(src, C.c_void_p), len(pkt), level)
    out = (C.c_char * max(cap, 1))()
    n = L.e264hip_packet_compact2(C.cast(src, C.c_void_p), len(pkt), level, C.cast(out, C.c_void_p), cap) if cap else 0
    if not n:
        raise BackendError(f"packet_compact: {last_error()}")
    return bytes(out[:n])


def packet_fold(pkt: bytes, level: int) -> bytes:
    """A version-4 packet folded at `level` of the WIRE form: 1 and 2 give the bytes of packet_compact, 3 gives version 7 (runs of equal plain entries
    travel as one entry).  Host only."""
    L = load_library()
    src = (C.c_char * len(pkt)).from_buffer_copy(pkt)
    cap = L.e264hip_packet_fold_bound(C.cast(src, C.c_void_p), len(pkt), level)
    out = (C.c_char * max(cap, 1))()
    n = L.e264hip_packet_fold(C.cast(src, C.c_void_p), len(pkt), level, C.cast(out, C.c_void_p), cap) if cap else 0
    if not n:
        raise BackendError(f"packet_fold: {last_error()}")
    return bytes(out[:n])


def packet_expand(pkt: bytes) -> bytes:
    """A wire packet as the canonical version-4 packet it stands for.  Host only."""
    L = load_library()
    src = (C.c_char * len(pkt)).from_buffer_copy(pkt)
    cap = L.e264hip_packet_expand(C.cast(src, C.c_void_p), len(pkt), None, 0)
    if not cap:
        raise BackendError(f"packet_expand: {last_error()}")
    out = (C.c_char * cap)()
    n = L.e264hip_packet_expand(C.cast(src, C.c_void_p), len(pkt), C.cast(out, C.c_void_p), cap)
    if not n:
        raise BackendError(f"packet_expand: {last_error()}")
    return bytes(out[:n])


def view_check(view, slot_bytes: int) -> int:
    """Host-only validation of a picture's view against a slot of slot_bytes (no GPU needed): 0 or an errno value."""
    return load_library().e264hip_view_check(C.byref(as_view(view)), slot_bytes)


def last_error() -> str:
    msg = load_library().e264hip_last_error()
    return msg.decode() if msg else ""


class Device:
    """One MI355X: queue + kernels (E264Device)."""

    def __init__(self, ordinal: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L, self.L.e264hip_device_open(ordinal, C.byref(h)), "e264hip_device_open")
        self.h = h
        self.ordinal = ordinal

    def close(self):
        if self.h:
            self.L.e264hip_device_close(self.h)
            self.h = None

    def sync(self):
        _check(self.L, self.L.e264hip_device_sync(self.h), "device_sync")

    def set_option(self, name: str, value: int) -> int:
        return self.L.e264hip_set_option(self.h, name.encode(), value)

    def launch_counts(self, reset: bool = False) -> dict:
        """Pictures per kernel form since the device was opened or last reset (LAUNCH_COUNT_NAMES), and the CU count as "n_cus"."""
        out = (C.c_uint64 * len(LAUNCH_COUNT_NAMES))()
        r = self.L.e264hip_launch_counts(self.h, out, len(out), int(reset))
        if r != len(LAUNCH_COUNT_NAMES):
            raise BackendError(f"e264hip_launch_counts: {r} slots, this binding knows {len(LAUNCH_COUNT_NAMES)}")
        return {k: int(v) for k, v in zip(LAUNCH_COUNT_NAMES, out)}

    def upload_packet(self, pkt: bytes) -> "DevicePacket":
        return DevicePacket(self, pkt)

    def submit_batch(self, streams, packets, mode: int = RUN_ALL) -> None:
        n = len(streams)
        sa = (C.c_void_p * n)(*[s.h for s in streams])
        pa = (C.c_void_p * n)(*[p.h for p in packets])
        _check(self.L, self.L.e264hip_submit_batch(self.h, sa, pa, n, mode), "submit_batch")

    def submit_batch_host(self, streams, packets, mode: int = RUN_ALL) -> None:
        """packets: bytes objects still in host memory (asynchronous: staged, copied and launched on the queue)."""
        n = len(streams)
        sa = (C.c_void_p * n)(*[s.h for s in streams])
        bufs = [(C.c_char * len(p)).from_buffer_copy(p) for p in packets]
        pa = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs])
        za = (C.c_size_t * n)(*[len(p) for p in packets])
        _check(self.L, self.L.e264hip_submit_batch_host(self.h, sa, pa, za, n, mode), "submit_batch_host")

    def prepare_host_batch(self, streams, packets):
        """The argument arrays of submit_batch_host built once (benchmarks re-submit the same host packets)."""
        n = len(streams)
        bufs = [(C.c_char * len(p)).from_buffer_copy(p) for p in packets]
        return ((C.c_void_p * n)(*[s.h for s in streams]), (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in bufs]),
                (C.c_size_t * n)(*[len(p) for p in packets]), n, bufs)

    def pinned_copy(self, pkt: bytes):
        """The packet's bytes in page-locked memory of this device (what a front end's emitter writes into directly)."""
        p = self.L.e264hip_host_alloc(self.h, len(pkt))
        if not p:
            raise BackendError("e264hip_host_alloc: " + last_error())
        C.memmove(p, pkt, len(pkt))
        return p

    def pinned_free(self, p) -> None:
        self.L.e264hip_host_free(self.h, p)

    def prepare_pinned_batch(self, streams, pinned_ptrs, sizes):
        n = len(streams)
        return ((C.c_void_p * n)(*[s.h for s in streams]), (C.c_void_p * n)(*pinned_ptrs), (C.c_size_t * n)(*sizes), n)

    def submit_pinned_prepared(self, pb, mode: int = RUN_ALL, trusted: bool = True) -> None:
        _check(self.L, self.L.e264hip_submit_batch_pinned(self.h, pb[0], pb[1], pb[2], pb[3], mode, 1 if trusted else 0), "submit_batch_pinned")

    def submit_host_prepared(self, hb, mode: int = RUN_ALL) -> None:
        _check(self.L, self.L.e264hip_submit_batch_host(self.h, hb[0], hb[1], hb[2], hb[3], mode), "submit_batch_host")

    def make_batch(self, streams, packets):
        """Device-resident job table for repeated launches (E264Batch)."""
        n = len(streams)
        sa = (C.c_void_p * n)(*[s.h for s in streams])
        pa = (C.c_void_p * n)(*[p.h for p in packets])
        b = C.c_void_p()
        _check(self.L, self.L.e264hip_batch_create(self.h, sa, pa, n, C.byref(b)), "batch_create")
        return b

    def submit_prepared(self, batch, mode: int = RUN_ALL) -> None:
        _check(self.L, self.L.e264hip_batch_submit(batch, mode), "batch_submit")

    def free_batch(self, batch) -> None:
        self.L.e264hip_batch_free(batch)

    def digest_batch(self, streams, slots, views) -> np.ndarray:
        """The digests (include/edge264_hip.h, version 1) of views[k] of slot slots[k] of streams[k], computed on the device behind everything
        queued on the streams' lane: an (n, 3) uint64 array, Y / Cb / Cr per row, in call order.  Blocks."""
        n = len(streams)
        if not (len(slots) == len(views) == n):
            raise ValueError("digest_batch: streams, slots and views differ in length")
        out = np.zeros((n, 3), np.uint64)
        sa = (C.c_void_p * max(n, 1))(*[s.h for s in streams])
        la = (C.c_int * max(n, 1))(*[int(x) for x in slots])
        va = (View * max(n, 1))(*[as_view(v) for v in views])
        _check(self.L, self.L.e264hip_digest_batch(self.h, sa, la, va, n, out.ctypes.data_as(C.POINTER(C.c_uint64))), "digest_batch")
        return out

    def diff_batch(self, streams_a, slots_a, views_a, streams_b, slots_b, views_b) -> np.ndarray:
        """The difference records (include/edge264_hip.h, version 1) of views_a[k] of slot slots_a[k] of streams_a[k] against views_b[k] of slot slots_b[k] of
        streams_b[k], computed on the device behind everything queued on the streams' lane, in one kernel.  Returns a structured array of shape (n, 3) and
        dtype DIFF_DTYPE: [k][p]["sad" | "sse" | "count" | "first" | "max"] for plane p = Y, Cb, Cr ("first" is DIFF_NONE for equal planes).  Blocks."""
        n = len(streams_a)
        if not (len(slots_a) == len(views_a) == len(streams_b) == len(slots_b) == len(views_b) == n):
            raise ValueError("diff_batch: the six lists differ in length")
        out = np.zeros((n, 3), DIFF_DTYPE)
        sa, sb = (C.c_void_p * n)(*[s.h for s in streams_a]), (C.c_void_p * n)(*[s.h for s in streams_b])
        la, lb = (C.c_int * n)(*slots_a), (C.c_int * n)(*slots_b)
        va, vb = (View * n)(*[as_view(v) for v in views_a]), (View * n)(*[as_view(v) for v in views_b])
        _check(self.L, self.L.e264hip_diff_batch(self.h, sa, la, va, sb, lb, vb, n, out.ctypes.data), "diff_batch")
        return out

    def hist_batch(self, streams, slots, views) -> np.ndarray:
        """The histogram records (include/edge264_hip.h, version 1) of views[k] of slot slots[k] of streams[k], computed on the device behind everything
        queued on the streams' lane, in one kernel: a uint32 array of shape (n, 3, 256), [k][p][v] = the samples of plane p = Y, Cb, Cr equal to v.  Blocks."""
        n = len(streams)
        if not (len(slots) == len(views) == n):
            raise ValueError("hist_batch: the three lists differ in length")
        out = np.zeros((n, 3, 256), np.uint32)
        sa = (C.c_void_p * n)(*[s.h for s in streams])
        la = (C.c_int * n)(*slots)
        va = (View * n)(*[as_view(v) for v in views])
        _check(self.L, self.L.e264hip_hist_batch(self.h, sa, la, va, n, out.ctypes.data), "hist_batch")
        return out

    def preview_batch(self, streams, slots, views, k: int = 3):
        """The previews (include/edge264_hip.h, version 1: box filter by 1 << k, k = 1, 2, 3) of views[i] of slot slots[i] of streams[i], computed on the
        device behind everything queued on the streams' lane: a list of [Y, Cb, Cr] 2-D uint8 arrays, in call order.  Blocks."""
        n = len(streams)
        if not (len(slots) == len(views) == n):
            raise ValueError("preview_batch: streams, slots and views differ in length")
        cv = [as_view(v) for v in views]
        dims = [preview_dims(v, k) for v in cv]
        pitch = max([sum(ow * oh for ow, oh in d) for d in dims], default=0)
        out = np.zeros((n, pitch), np.uint8)
        sa = (C.c_void_p * max(n, 1))(*[s.h for s in streams])
        la = (C.c_int * max(n, 1))(*[int(x) for x in slots])
        va = (View * max(n, 1))(*cv)
        _check(self.L, self.L.e264hip_preview_batch(self.h, sa, la, va, n, k, out.ctypes.data, pitch), "preview_batch")
        return [_split_preview(out[j], dims[j]) for j in range(n)]

    def blockdiff_batch(self, streams_a, slots_a, views_a, streams_b, slots_b, views_b, k: int = 4):
        """The block difference maps (include/edge264_hip.h, version 1: blocks of 1 << k, k = 3 .. 6) of views_a[i] of slot slots_a[i] of streams_a[i] against
        views_b[i] of slot slots_b[i] of streams_b[i], computed on the device behind everything queued on the streams' lane, in one kernel: a list of
        [Y, Cb, Cr] 2-D arrays of dtype BLOCKDIFF_DTYPE and shape (bh, bw) ("sad", "sse"), in call order.  Blocks."""
        n = len(streams_a)
        if not (len(slots_a) == len(views_a) == len(streams_b) == len(slots_b) == len(views_b) == n):
            raise ValueError("blockdiff_batch: the six lists differ in length")
        ca, cb = [as_view(v) for v in views_a], [as_view(v) for v in views_b]
        dims = [blockdiff_dims(v, k) for v in ca]
        pitch = max([sum(8 * bw * bh for bw, bh in d) for d in dims], default=0)
        out = np.zeros((n, pitch), np.uint8)
        m = max(n, 1)
        sa, sb = (C.c_void_p * m)(*[s.h for s in streams_a]), (C.c_void_p * m)(*[s.h for s in streams_b])
        la, lb = (C.c_int * m)(*[int(x) for x in slots_a]), (C.c_int * m)(*[int(x) for x in slots_b])
        va, vb = (View * m)(*ca), (View * m)(*cb)
        _check(self.L, self.L.e264hip_blockdiff_batch(self.h, sa, la, va, sb, lb, vb, n, k, out.ctypes.data, pitch), "blockdiff_batch")
        return [_split_blockdiff(out[j], dims[j]) for j in range(n)]

    def blockstat_batch(self, streams, slots, views, k: int = 4):
        """The block statistics maps (include/edge264_hip.h, version 1: blocks of 1 << k, k = 3 .. 6) of views[i] of slot slots[i] of streams[i], computed on the
        device behind everything queued on the streams' lane, in one kernel: a list of [Y, Cb, Cr] 2-D arrays of dtype BLOCKSTAT_DTYPE and shape (bh, bw)
        ("sum", "sumsq", "gh", "gv"), in call order.  Blocks."""
        n = len(streams)
        if not (len(slots) == len(views) == n):
            raise ValueError("blockstat_batch: streams, slots and views differ in length")
        cv = [as_view(v) for v in views]
        dims = [blockstat_dims(v, k) for v in cv]
        pitch = max([sum(16 * bw * bh for bw, bh in d) for d in dims], default=0)
        out = np.zeros((n, pitch), np.uint8)
        m = max(n, 1)
        sa = (C.c_void_p * m)(*[s.h for s in streams])
        la = (C.c_int * m)(*[int(x) for x in slots])
        va = (View * m)(*cv)
        _check(self.L, self.L.e264hip_blockstat_batch(self.h, sa, la, va, n, k, out.ctypes.data, pitch), "blockstat_batch")
        return [_split_blockstat(out[j], dims[j]) for j in range(n)]

    def event_record(self, idx: int) -> None:
        _check(self.L, self.L.e264hip_event_record(self.h, idx), "event_record")

    def event_elapsed_ms(self, a: int, b: int) -> float:
        ms = C.c_float()
        _check(self.L, self.L.e264hip_event_elapsed_ms(self.h, a, b, C.byref(ms)), "event_elapsed")
        return float(ms.value)

    def event_done(self, idx: int) -> bool:
        """Has everything queued before event_record(idx) left the GPU?  Never blocks."""
        r = self.L.e264hip_event_query(self.h, idx)
        if r not in (0, errno.EBUSY):
            _check(self.L, r, "event_query")
        return r == 0

    def kernel_timing(self, enable: bool) -> None:
        _check(self.L, self.L.e264hip_kernel_timing(self.h, int(enable)), "kernel_timing")

    def kernel_time_ms(self):
        t, n = (C.c_double * 4)(), C.c_int()
        _check(self.L, self.L.e264hip_kernel_time_ms(self.h, t, C.byref(n)), "kernel_time")
        return [float(x) for x in t], int(n.value)


class DevicePacket:
    def __init__(self, dev: Device, pkt: bytes):
        self.dev, self.nbytes = dev, len(pkt)
        h = C.c_void_p()
        buf = (C.c_char * len(pkt)).from_buffer_copy(pkt)
        _check(dev.L, dev.L.e264hip_packet_upload(dev.h, C.cast(buf, C.c_void_p), len(pkt), C.byref(h)), "packet_upload")
        self.h = h

    def free(self):
        if self.h:
            self.dev.L.e264hip_packet_free(self.h)
            self.h = None


class Stream:
    """Device side of one decoder (E264Stream): DPB slots in HBM."""

    def __init__(self, dev: Device, width_mbs: int, height_mbs: int):
        self.dev, self.L = dev, dev.L
        self.w, self.h_mbs = width_mbs, height_mbs
        self.frame_bytes = P.frame_bytes(width_mbs, height_mbs)
        h = C.c_void_p()
        _check(self.L, self.L.e264hip_stream_open(dev.h, C.byref(h)), "stream_open")
        self.h = h

    def close(self):
        if self.h:
            self.L.e264hip_stream_close(self.h)
            self.h = None

    def bind_lane(self, lane: int) -> None:
        """Compute lane (HIP queue) of the device this stream's work is ordered on; streams of different lanes overlap."""
        _check(self.L, self.L.e264hip_stream_bind_lane(self.h, lane), "stream_bind_lane")

    def alloc(self, slot: int, mirror: bool = False) -> None:
        m = C.c_void_p()
        _check(self.L, self.L.e264hip_frame_alloc(self.h, slot, self.frame_bytes, C.byref(m) if mirror else None), "frame_alloc")

    def free(self, slot: int) -> None:
        self.L.e264hip_frame_free(self.h, slot)

    def fill(self, slot: int, value: int) -> None:
        _check(self.L, self.L.e264hip_frame_fill(self.h, slot, value), "frame_fill")

    def upload(self, slot: int, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, np.uint8)
        _check(self.L, self.L.e264hip_frame_upload(self.h, slot, data.ctypes.data, min(data.nbytes, self.frame_bytes)), "frame_upload")

    def submit(self, pkt: bytes) -> None:
        buf = (C.c_char * len(pkt)).from_buffer_copy(pkt)
        _check(self.L, self.L.e264hip_frame_submit(self.h, C.cast(buf, C.c_void_p), len(pkt)), "frame_submit")

    def download(self, slot: int) -> np.ndarray:
        out = np.empty(self.frame_bytes, np.uint8)
        _check(self.L, self.L.e264hip_frame_download(self.h, slot, out.ctypes.data, out.nbytes), "frame_download")
        return out

    def digest(self, slot: int, view=None):
        """(Y, Cb, Cr) digests of the picture in `slot`, computed on the device behind everything queued for the stream (a submission, a fill): three
        ints.  view: where the picture lies (digest.frame_view; a backend.View); default the whole picture in the reference's layout.  Blocks."""
        if view is None:
            from .digest import frame_view
            view = frame_view(self.w, self.h_mbs)
        out = (C.c_uint64 * 3)()
        _check(self.L, self.L.e264hip_frame_digest(self.h, slot, C.byref(as_view(view)), out), "frame_digest")
        return tuple(int(x) for x in out)

    def diff(self, slot: int, view=None, other=None, other_slot=None, other_view=None) -> np.ndarray:
        """The difference record of the picture in `slot` against the picture in `other_slot` of stream `other` (default: this stream, the same slot),
        computed on the device behind everything queued for the streams: a structured array of shape (3,) and dtype DIFF_DTYPE (Y, Cb, Cr).  view,
        other_view: as for digest; default the whole picture of each stream in the reference's layout.  Blocks."""
        from .digest import frame_view
        other = self if other is None else other
        other_slot = slot if other_slot is None else other_slot
        if view is None:
            view = frame_view(self.w, self.h_mbs)
        if other_view is None:
            other_view = frame_view(other.w, other.h_mbs)
        out = np.zeros(3, DIFF_DTYPE)
        _check(self.L, self.L.e264hip_frame_diff(self.h, slot, C.byref(as_view(view)), other.h, other_slot, C.byref(as_view(other_view)), out.ctypes.data), "frame_diff")
        return out

    def hist(self, slot: int, view=None) -> np.ndarray:
        """The histogram record of the picture in `slot`, computed on the device behind everything queued for the stream: a uint32 array of shape
        (3, 256), [p][v] = the samples of plane p = Y, Cb, Cr equal to v.  view: as for digest; default the whole picture in the reference's layout.  Blocks."""
        from .digest import frame_view
        if view is None:
            view = frame_view(self.w, self.h_mbs)
        out = np.zeros((3, 256), np.uint32)
        _check(self.L, self.L.e264hip_frame_hist(self.h, slot, C.byref(as_view(view)), out.ctypes.data), "frame_hist")
        return out

    def blockdiff(self, slot: int, view=None, other=None, other_slot=None, other_view=None, k: int = 4):
        """The block difference map (blocks of 1 << k, k = 3 .. 6) of the picture in `slot` against the picture in `other_slot` of stream `other` (default: this
        stream, the same slot), computed on the device behind everything queued for the streams: [Y, Cb, Cr] 2-D arrays of dtype BLOCKDIFF_DTYPE and shape
        (bh, bw).  view, other_view: as for diff; default the whole picture of each stream in the reference's layout.  Blocks."""
        from .digest import frame_view
        other = self if other is None else other
        other_slot = slot if other_slot is None else other_slot
        if view is None:
            view = frame_view(self.w, self.h_mbs)
        if other_view is None:
            other_view = frame_view(other.w, other.h_mbs)
        cv = as_view(view)
        dims = blockdiff_dims(cv, k)
        out = np.zeros(sum(8 * bw * bh for bw, bh in dims), np.uint8)
        _check(self.L, self.L.e264hip_frame_blockdiff(self.h, slot, C.byref(cv), other.h, other_slot, C.byref(as_view(other_view)), k, out.ctypes.data, out.nbytes), "frame_blockdiff")
        return _split_blockdiff(out, dims)

    def blockstat(self, slot: int, view=None, k: int = 4):
        """The block statistics map (blocks of 1 << k, k = 3 .. 6) of the picture in `slot`, computed on the device behind everything queued for the stream:
        [Y, Cb, Cr] 2-D arrays of dtype BLOCKSTAT_DTYPE and shape (bh, bw).  view: as for digest; default the whole picture in the reference's layout.  Blocks."""
        from .digest import frame_view
        if view is None:
            view = frame_view(self.w, self.h_mbs)
        cv = as_view(view)
        dims = blockstat_dims(cv, k)
        out = np.zeros(sum(16 * bw * bh for bw, bh in dims), np.uint8)
        _check(self.L, self.L.e264hip_frame_blockstat(self.h, slot, C.byref(cv), k, out.ctypes.data, out.nbytes), "frame_blockstat")
        return _split_blockstat(out, dims)

    def preview(self, slot: int, view=None, k: int = 3):
        """[Y, Cb, Cr] of the picture in `slot` reduced by 1 << k (k = 1, 2, 3) in each direction, computed on the device behind everything queued for the
        stream: three 2-D uint8 arrays.  view: as for digest; default the whole picture in the reference's layout.  Blocks."""
        if view is None:
            from .digest import frame_view
            view = frame_view(self.w, self.h_mbs)
        cv = as_view(view)
        dims = preview_dims(cv, k)
        out = np.zeros(sum(ow * oh for ow, oh in dims), np.uint8)
        _check(self.L, self.L.e264hip_frame_preview(self.h, slot, C.byref(cv), k, out.ctypes.data, out.nbytes), "frame_preview")
        return _split_preview(out, dims)

    def flush(self) -> None:
        _check(self.L, self.L.e264hip_stream_flush(self.h), "stream_flush")
