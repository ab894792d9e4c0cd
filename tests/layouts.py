"""Padded picture layouts for the tests (not a conftest: imported by the tests that use it).

A packet's header says where the samples lie in a slot: stride_Y, stride_C, plane_size_Y and plane_size_C (include/edge264_cmd.h).
The front end and the synthesiser emit the reference's tight layout (packet.frame_geometry), where a store past the end of a row lands
in the next row's samples and one past the last luma row lands in Cb.  The layouts below put padding right of every row and gaps behind
the planes, so that a kernel that writes a byte that is not a sample of the picture, or whose output depends on one, changes a byte
the tests can see.

A layout is (pad_y, pad_c, gap_y, gap_c), added to the tight geometry: stride_Y + pad_y, stride_C + pad_c, plane_size_Y = stride_Y *
rows + gap_y, plane_size_C = stride_C * rows / 2 + gap_c.  A slot holds plane_size_Y + plane_size_C bytes and a guard of guard_bytes()
behind them, all random before a picture is decoded into it.
"""
import numpy as np

from edge264_amd import backend, packet as P

LAYOUTS = {
    "tight": (0, 0, 0, 0),
    "pad16": (16, 8, 0, 0),            # Cr rows only 4-byte aligned (Cb + stride_C / 2)
    "pad_wide": (48, 24, 0, 0),
    "pad_wider": (256, 136, 0, 0),
    "gaps": (0, 0, 16, 4112),          # a small gap behind luma, 4096 + 16 bytes behind chroma
    "gaps_wide": (16, 8, 4112, 8),     # 4096 + 16 bytes behind luma, a small gap behind chroma
    "canvas": (4096, 4104, 0, 0),      # a narrow picture in a wide canvas (stride_Y = 4096 + 16 for 1 macroblock)
}
PADDED = [k for k in LAYOUTS if k != "tight"]
# the layouts of the streams of one batch, in turn (the "mixed" batch: each stream its own layout)
MIXED = ["pad16", "canvas", "gaps", "tight", "pad_wider", "gaps_wide", "pad_wide"]


def geometry(width_mbs, height_mbs, layout):
    """the four header fields of a picture in a layout (a name of LAYOUTS or a tuple)"""
    pad_y, pad_c, gap_y, gap_c = LAYOUTS[layout] if isinstance(layout, str) else layout
    g = P.frame_geometry(width_mbs, height_mbs)
    sy, sc = g["stride_Y"] + pad_y, g["stride_C"] + pad_c
    return dict(stride_Y=sy, stride_C=sc, plane_size_Y=sy * height_mbs * 16 + gap_y, plane_size_C=sc * height_mbs * 8 + gap_c)


def restride(pkt, pad_y, pad_c, gap_y, gap_c, check=True) -> bytes:
    """a version-4 or wire packet with its picture in another layout: stride_Y, stride_C, plane_size_Y and plane_size_C rewritten, every
    other byte as it was; the validator accepts it (check=False: the caller asserts the verdict)"""
    buf = bytearray(pkt)
    h = np.frombuffer(buf, P.FRAME_HDR, 1)
    for k, v in geometry(int(h["width_mbs"][0]), int(h["height_mbs"][0]), (pad_y, pad_c, gap_y, gap_c)).items():
        h[k] = v
    out = bytes(buf)
    if check:
        assert backend.packet_check(out) == 0, (pad_y, pad_c, gap_y, gap_c, backend.last_error())
    return out


def in_layout(pkt, layout) -> bytes:
    return restride(pkt, *(LAYOUTS[layout] if isinstance(layout, str) else layout))


def hdr_of(pkt):
    """the header fields (a wire packet's too: the header is shared), as ints"""
    h = np.frombuffer(pkt, P.FRAME_HDR, 1)[0]
    return {k: int(h[k]) for k in ("width_mbs", "height_mbs", "stride_Y", "stride_C", "plane_size_Y", "plane_size_C", "dst_slot", "ref_slots")}


def guard_bytes(hdr) -> int:
    """the guard behind plane_size_C: at least 4096 bytes and at least one luma row"""
    return max(4096, hdr["stride_Y"])


def slot_bytes(hdr) -> int:
    return hdr["plane_size_Y"] + hdr["plane_size_C"] + guard_bytes(hdr)


def sample_mask(hdr, n=None):
    """the bytes of a slot of n bytes (default slot_bytes) that are samples of the picture: luma W x H at stride_Y; Cb and Cr W/2 x H/2 each
    at stride_C from plane_size_Y, Cr at + stride_C / 2.  No other byte of a slot may change."""
    n = slot_bytes(hdr) if n is None else n
    W, H = hdr["width_mbs"] * 16, hdr["height_mbs"] * 16
    sy, sc, psy = hdr["stride_Y"], hdr["stride_C"], hdr["plane_size_Y"]
    m = np.zeros(n, bool)
    m[:sy * H].reshape(H, sy)[:, :W] = True
    c = m[psy:psy + sc * (H // 2)].reshape(H // 2, sc)
    c[:, :W // 2] = True
    c[:, sc // 2:sc // 2 + W // 2] = True
    return m


def samples(hdr, slot):
    """(luma H x W, chroma H/2 x W: [Cb | Cr]) views of a slot's samples"""
    W, H = hdr["width_mbs"] * 16, hdr["height_mbs"] * 16
    sy, sc, psy = hdr["stride_Y"], hdr["stride_C"], hdr["plane_size_Y"]
    y = slot[:sy * H].reshape(H, sy)[:, :W]
    c = slot[psy:psy + sc * (H // 2)].reshape(H // 2, sc)
    return y, np.concatenate([c[:, :W // 2], c[:, sc // 2:sc // 2 + W // 2]], axis=1)


def random_slot(hdr, rng, samples_from=None):
    """a slot's full image: random bytes everywhere (picture, padding, gaps and guard); with samples_from (a slot of the same layout) its
    samples copied in"""
    a = rng.integers(0, 256, slot_bytes(hdr), dtype=np.uint8)
    if samples_from is not None:
        m = sample_mask(hdr, len(a))
        a[m] = samples_from[:len(a)][m]
    return a


def first_difference(hdr, got, want, what):
    """a readable position of the first differing byte of a slot: plane, row, column, and whether it is a sample"""
    i = int(np.argmax(got != want))
    sy, sc, psy, psc = hdr["stride_Y"], hdr["stride_C"], hdr["plane_size_Y"], hdr["plane_size_C"]
    W, H = hdr["width_mbs"] * 16, hdr["height_mbs"] * 16
    if i < psy:
        where = f"luma row {i // sy} column {i % sy}" + ("" if i // sy < H and i % sy < W else " (padding / gap)")
    elif i < psy + psc:
        r, c = divmod(i - psy, sc)
        pl, c = ("Cr", c - sc // 2) if c >= sc // 2 else ("Cb", c)
        where = f"{pl} row {r} column {c}" + ("" if r < H // 2 and 0 <= c < W // 2 else " (padding / gap)")
    else:
        where = f"guard byte {i - psy - psc}"
    n = int((got != want).sum())
    return f"{what}: {n} bytes differ, the first at byte {i} = {where}: {int(got[i])} instead of {int(want[i])}"
