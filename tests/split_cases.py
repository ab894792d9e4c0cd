"""Pictures that reach the back end in SEVERAL packets, cut where the kernels hand work over: inside a 16 x 4 tile of the prediction kernel, between
two 64-macroblock chunks of the intra kernel's wavefront, between two row groups of the deblocking kernel (not a conftest: imported by the tests that
use it, like tests/structure_cases.py).

What a packet of a split picture looks like, from include/edge264_cmd.h (E264_MB_ABSENT, E264_MBF_DONE) and from what the front end does to the
records of a picture one of whose slices failed (edge264_amd/frontend/edge264_hip_frontend.c, "a picture in several packets"):
- every packet of the picture carries the whole record table, the motion section and the slice table;
- a macroblock that has not arrived yet is E264_MB_ABSENT: its samples are left as they are, nothing is deblocked there;
- a macroblock that an EARLIER packet of the picture reconstructed keeps its record for its neighbours (bS, QP averages) with E264_MBF_DONE set,
  coded = 0 and payload_off = 0: nothing reconstructs it again, it has no payload;
- E264_MBF_DEBLOCK, E264_MBF_EDGE_LEFT and E264_MBF_EDGE_TOP stand only on the macroblocks THIS packet deblocks; a macroblock is deblocked by exactly
  one packet of its picture, which may be a later one than the packet that reconstructed it (it is then DONE and deblocked);
- the header's n_coded_mbs, n_inter_mbs and ref_slots follow the records (DONE ones count by their kind);
- the motion and payload sections stay as they are: bytes no record points to any more are what the front end leaves behind too.

split() derives such packets from one tight version-4 packet.  r[a] is the packet that reconstructs macroblock a.  d[a], the packet that deblocks it,
is r[a] raised to r of the left neighbour where the record filters its left edge, to r of the top neighbour where it filters its top edge (an edge is
filtered once both of its sides are there) and to delay[a] where a delay is given.  In packet k: r > k is ABSENT, r < k is DONE, d != k clears the
three deblocking flags.

The shapes are functions (W, H) -> (n_packets, r, delay).  A census counts per packet, from the packet alone, what each shape is named after, and
packets() asserts the shape's minimum counts wherever packets are made, so that a later change to the generator cannot hollow a case out.  The sizes
written out here, not taken from the kernel headers: a tile is 16 x 4 macroblocks, a chunk of the intra kernel 64 macroblocks of a row, a row group of
the deblocking kernel 5 rows (luma and chroma together), 8 rows (luma alone) or 15 or 16 rows (chroma alone, by build)."""
import functools
from collections import Counter

import numpy as np

from edge264_amd import backend, packet as P, synth

TILE_W, TILE_H, CHUNK = 16, 4, 64
ALL_I = (P.MB_I4x4, P.MB_I8x8, P.MB_I16x16)
DBK_FLAGS = P.MBF_DEBLOCK | P.MBF_EDGE_LEFT | P.MBF_EDGE_TOP
GEOMS = [(17, 5), (66, 9), (130, 5), (5, 17)]
PATTERN = "IPBP"


# ---- one picture into packets ----------------------------------------------------------------------------------------------------------------------

def deblocked_by(raw, r, delay=None) -> np.ndarray:
    """d[a]: the packet that deblocks macroblock a"""
    pk = P.Packet(bytes(raw))
    W = pk.width_mbs
    r = np.asarray(r, np.int64).reshape(-1)
    flags = pk.mbs["flags"].astype(int)
    d = r.copy()
    for a in range(len(r)):
        if flags[a] & P.MBF_EDGE_LEFT:
            d[a] = max(d[a], r[a - 1])
        if flags[a] & P.MBF_EDGE_TOP:
            d[a] = max(d[a], r[a - W])
    if delay is not None:
        d = np.maximum(d, np.asarray(delay, np.int64).reshape(-1))
    return d


def split(raw, r, n_packets, delay=None) -> list:
    """the n_packets packets of the picture of the tight version-4 packet `raw` (every macroblock present, none DONE), each accepted by the validator"""
    raw = bytes(raw)
    pk = P.Packet(raw)
    n = len(pk.mbs)
    assert int(pk.hdr["version"]) == P.E264_VERSION and (pk.mbs["kind"] != P.MB_ABSENT).all() and not (pk.mbs["flags"] & P.MBF_DONE).any()
    r = np.asarray(r, np.int64).reshape(-1)
    d = deblocked_by(raw, r, delay)
    assert len(r) == n and r.min() >= 0 and d.max() < n_packets
    out = []
    for k in range(n_packets):
        buf = bytearray(raw)
        mbs = np.frombuffer(buf, P.MB, n, int(pk.hdr["mbs_off"]))
        later, earlier, not_now = r > k, r < k, d != k
        mbs["kind"][later] = P.MB_ABSENT
        mbs["flags"][earlier] |= P.MBF_DONE
        mbs["coded"][earlier] = 0
        mbs["payload_off"][earlier] = 0
        mbs["flags"][later | not_now] &= 0xff ^ DBK_FLAGS
        del mbs
        P.refresh_summary(buf)
        p = bytes(buf)
        assert backend.packet_check(p) == 0, (k, backend.last_error())
        out.append(p)
    return out


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------------------

def cut_column(W) -> int:
    """the column a vertical cut lies on: the chunk boundary where the picture has one, else the tile boundary, else the middle"""
    return CHUNK if W > CHUNK else TILE_W if W > TILE_W else W // 2 + 1


def raster(W, H, cuts):
    """raster prefixes: packet k reconstructs the macroblocks from cut k - 1 up to cut k"""
    cuts = sorted(set(int(c) for c in cuts))
    assert cuts and 0 < cuts[0] and cuts[-1] < W * H
    return len(cuts) + 1, np.searchsorted(np.array(cuts), np.arange(W * H), side="right"), None


def raster_split(raw, W, H, cuts) -> list:
    """the picture's packets when it is cut at `cuts` in raster order"""
    n_packets, r, delay = raster(W, H, cuts)
    return split(raw, r, n_packets, delay)


def raster_cuts(W, H) -> dict:
    """the places a raster cut is taken at (name -> first macroblock behind the cut)"""
    c = {"one": 1, "mid_row": W + W // 2, "last": W * H - 1}
    if W > TILE_W:
        c["x16"] = 2 * W + TILE_W
    if W > CHUNK:
        c["x64"] = 3 * W + CHUNK
    for y in [y for y in (5, 8, 15, 16) if y < H] or [3]:  # row starts: between two row groups where the picture has two
        c[f"row{y}"] = y * W
    return c


def raster_cut(W, H):
    return raster(W, H, raster_cuts(W, H).values())


def cut_sets(W, H) -> list:
    """every raster cut alone (two packets) and every two neighbouring ones together (three): the splits that must not show"""
    cuts = sorted(raster_cuts(W, H).values())
    return [(c,) for c in cuts] + list(zip(cuts, cuts[1:]))


def two_cut_places(W, H) -> list:
    return [(H // 3) * W + W // 3, (2 * H // 3) * W + 2 * W // 3]


def two_cuts(W, H):
    return raster(W, H, two_cut_places(W, H))


def hole_ends(W, H) -> tuple:
    """the run that arrives last: from the cut column of row H / 3 up to the cut column of row 2 H / 3 (at least a row under it has arrived before)"""
    x = cut_column(W) % W
    a, b = (H // 3) * W + x, (2 * H // 3) * W + x
    assert 0 < a and a + W <= b and b + W <= W * H
    return a, b


def hole(W, H):
    a, b = hole_ends(W, H)
    addr = np.arange(W * H)
    return 2, ((addr >= a) & (addr < b)).astype(np.int64), None


def checker(W, H):
    y, x = np.divmod(np.arange(W * H), W)
    return 2, (x + y) & 1, None


def columns(W, H):
    return 2, (np.arange(W * H) % W >= cut_column(W)).astype(np.int64), None


def late_deblock(W, H):
    return 2, np.zeros(W * H, np.int64), np.ones(W * H, np.int64)


SHAPES = dict(raster_cut=raster_cut, two_cuts=two_cuts, hole=hole, checker=checker, columns=columns, late_deblock=late_deblock)


# ---- the census ------------------------------------------------------------------------------------------------------------------------------------

def census(pkt) -> Counter:
    """one packet: fresh / done / absent records; done_deblocked: DONE macroblocks deblocked now; intra_below_done: fresh intra macroblocks with a DONE
    intra macroblock straight above; mixed_tiles: tiles with fresh and DONE macroblocks; pair_63_64: rows whose columns 63 and 64 are one DONE, one
    fresh; done_pcm: DONE I_PCM macroblocks; deblocked: macroblocks deblocked now"""
    pk = P.Packet(bytes(pkt))
    W, H = pk.width_mbs, pk.height_mbs
    kind = pk.mbs["kind"].astype(int).reshape(H, W)
    flags = pk.mbs["flags"].astype(int).reshape(H, W)
    absent = kind == P.MB_ABSENT
    done = (flags & P.MBF_DONE) != 0
    assert not (absent & done).any()
    fresh = ~absent & ~done
    intra = np.isin(kind, ALL_I)
    c = Counter(fresh=int(fresh.sum()), done=int(done.sum()), absent=int(absent.sum()),
                deblocked=int(((flags & P.MBF_DEBLOCK) != 0).sum()), done_deblocked=int((done & ((flags & P.MBF_DEBLOCK) != 0)).sum()),
                intra_below_done=int((fresh[1:] & intra[1:] & done[:-1] & intra[:-1]).sum()), done_pcm=int((done & (kind == P.MB_PCM)).sum()),
                fresh_intra=int((fresh & intra).sum()), fresh_inter=int((fresh & (kind == P.MB_INTER)).sum()))
    for ty in range(0, H, TILE_H):
        for tx in range(0, W, TILE_W):
            c["mixed_tiles"] += int(fresh[ty:ty + TILE_H, tx:tx + TILE_W].any() and done[ty:ty + TILE_H, tx:tx + TILE_W].any())
    if W > CHUNK:
        c["pair_63_64"] = int(((done[:, CHUNK - 1] & fresh[:, CHUNK]) | (fresh[:, CHUNK - 1] & done[:, CHUNK])).sum())
    # the record rules of the module's docstring, on every packet
    assert not (flags[absent] & DBK_FLAGS).any() and not pk.mbs["coded"].reshape(H, W)[done].any() and not pk.mbs["payload_off"].reshape(H, W)[done].any()
    assert int(pk.hdr["n_coded_mbs"]) == int((~absent).sum()) and int(pk.hdr["n_inter_mbs"]) == int((kind == P.MB_INTER).sum())
    return c


def _raster_minimum(W, H, cuts, N) -> dict:
    """packet j of a raster split: the macroblocks before cut j - 1 DONE, those from cut j on ABSENT; the tile with cut j - 1 holds both kinds unless
    the cut is the start of a row of tiles"""
    n, cuts = W * H, sorted(set(cuts))
    return dict(packets=N * (len(cuts) + 1), done=N * sum(cuts), absent=N * sum(n - c for c in cuts),
                mixed_tiles=N * sum(c % (TILE_H * W) != 0 for c in cuts))


def minimum(shape, stream, W, H) -> dict:
    """What the packets of one base stream (its four pictures together) must show at least.  Counted by hand from the shape: n macroblocks a picture,
    N = 4 pictures, every macroblock deblocked with both outer edges where the picture has them (the base streams filter across slices); the counts
    that depend on the generator's draws (intra over intra, I_PCM) are asked to occur at all."""
    n, N, wide = W * H, len(PATTERN), W > CHUNK
    tiles = [(min(TILE_W, W - tx), min(TILE_H, H - ty)) for ty in range(0, H, TILE_H) for tx in range(0, W, TILE_W)]
    if shape == "raster_cut":
        return dict(_raster_minimum(W, H, raster_cuts(W, H).values(), N), pair_63_64=N * wide, done_pcm=1, intra_below_done=1)
    if shape == "two_cuts":
        return dict(_raster_minimum(W, H, two_cut_places(W, H), N), done_pcm=1, intra_below_done=1)
    if shape == "hole":
        a, b = hole_ends(W, H)
        # the W macroblocks behind the hole were reconstructed before the one above them: their top edges wait for the hole's packet; columns 63 and
        # 64 differ in the hole's first and last row
        inside = ((np.arange(n) >= a) & (np.arange(n) < b)).reshape(H, W)
        both = sum(len(set(inside[ty:ty + TILE_H, tx:tx + TILE_W].ravel().tolist())) == 2 for ty in range(0, H, TILE_H) for tx in range(0, W, TILE_W))
        return dict(packets=N * 2, done=N * (n - (b - a)), absent=N * (b - a), mixed_tiles=N * both, pair_63_64=N * 2 * wide, done_pcm=1,
                    done_deblocked=N * W, intra_below_done=1)
    if shape == "checker":
        # every macroblock of the first packet but the picture's first has its left or its top edge to wait for; every tile of more than one
        # macroblock holds both kinds; straight above every macroblock of the second packet lies one of the first
        return dict(packets=N * 2, done=N * ((n + 1) // 2), absent=N * (n // 2), mixed_tiles=N * sum(w * h > 1 for w, h in tiles),
                    pair_63_64=N * H * wide, done_pcm=1, done_deblocked=N * ((n + 1) // 2 - 1), intra_below_done=n // 4)
    if shape == "columns":
        c = cut_column(W)
        # (a cut on a tile boundary: whole DONE tiles beside whole fresh ones)
        return dict(packets=N * 2, done=N * H * c, absent=N * H * (W - c), mixed_tiles=N * ((H + 3) // 4) * (c % TILE_W != 0), pair_63_64=N * H * wide,
                    done_pcm=1)
    if shape == "late_deblock":
        return dict(packets=N * 2, done=N * n, done_deblocked=N * n, fresh_in_last=0, done_pcm=1)
    raise KeyError(shape)


# ---- the base streams ------------------------------------------------------------------------------------------------------------------------------

def _pcm_places(x, y, W, H):
    """I_PCM on a lattice that meets every shape's DONE part (the first macroblock among them), inter elsewhere"""
    return "pcm" if (3 * x + 5 * y) % 11 == 0 else "inter"


_RICH = dict(t8x8=True, i_kinds=ALL_I, intra_in_inter=0.3, pcm_prob=0.05, residual_prob=0.6, slices_per_frame=3)
STREAMS = {
    "rich": _RICH,
    "inter": dict(_RICH, intra_in_inter=0.0, pcm_prob=0.0, place=_pcm_places, filter_offsets=(4, -2)),
}


def seed_of(stream, w, h) -> int:
    # (4002: the first base from 4000 on with which the rich stream has a DONE I_PCM macroblock in every shape at 6 x 5 macroblocks too)
    return 4002 + 1000 * list(STREAMS).index(stream) + 7 * w + h


@functools.lru_cache(maxsize=None)
def base(stream, w, h, deblock=True) -> tuple:
    """the base stream's tight packets (I P B P), made once per process"""
    g = synth.StreamSynth(w, h, seed_of(stream, w, h), **dict(STREAMS[stream], deblock=deblock))
    out = tuple(bytes(g.next_frame(t)) for t in PATTERN)
    assert all(backend.packet_check(p) == 0 for p in out)
    return out


def check_minimum(shape, stream, w, h, cens) -> Counter:
    """cens: per picture, the census of each of its packets"""
    total = Counter(packets=sum(len(c) for c in cens))
    for c in cens:
        for k in c:
            total.update(k)
        total["fresh_in_last"] += c[-1]["fresh"]
    least = minimum(shape, stream, w, h)
    assert all(total[k] >= v for k, v in least.items() if k != "fresh_in_last"), (shape, stream, w, h, {k: (total[k], v) for k, v in least.items()})
    if "fresh_in_last" in least:
        assert total["fresh_in_last"] == least["fresh_in_last"], (shape, stream, w, h, total)
    assert total["fresh"] == len(PATTERN) * w * h  # every macroblock reconstructed by exactly one packet
    return total


@functools.lru_cache(maxsize=None)
def packets(shape, stream, w, h) -> tuple:
    """every picture of the base stream split by the shape: (per picture, its packets), made once per process, the census held against the minimum"""
    n_packets, r, delay = SHAPES[shape](w, h)
    out = tuple(tuple(split(raw, r, n_packets, delay)) for raw in base(stream, w, h))
    # (the deblocking flags: every macroblock the unsplit packet deblocks is deblocked by exactly one packet)
    for raw, pkts in zip(base(stream, w, h), out):
        want = (P.Packet(raw).mbs["flags"] & DBK_FLAGS).astype(int)
        got = sum((P.Packet(p).mbs["flags"] & DBK_FLAGS).astype(int) for p in pkts)
        assert np.array_equal(want, got), (shape, stream, w, h)
    check_minimum(shape, stream, w, h, [[census(p) for p in pkts] for pkts in out])
    return out


def totals(shape, stream, w, h) -> Counter:
    return check_minimum(shape, stream, w, h, [[census(p) for p in pkts] for pkts in packets(shape, stream, w, h)])


def flat(per_picture) -> tuple:
    """(packets in order, a label for each: picture type and packet number)"""
    return ([p for pkts in per_picture for p in pkts], [f"{t}.{k}" for t, pkts in zip(PATTERN, per_picture) for k in range(len(pkts))])
