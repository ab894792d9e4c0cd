"""Pictures whose STRUCTURE reaches a capacity or a hand-off boundary inside a kernel (the range ends are tests/edge_cases.py's): class lists
of the prediction kernel filled to the last slot, two classes meeting inside the array they share, residual lists as full as a tile can make
them; intra macroblocks placed where the intra kernel's wavefront crosses a 64-macroblock chunk, where a chunk or a whole row is empty, where
the only macroblock to wait for is the one diagonally above; picture heights around the deblocking kernel's row groups.

A census counts, from the packet alone (edge264_amd/packet.py), what each case is named after; every test asserts it, so a later change to the
generator cannot hollow a case out unnoticed.  The rules are written out here, not taken from the kernel headers:
- a tile is 16 x 4 macroblocks.  Per tile and list, a quadrant (8x8) that the list predicts is 1 item if its four 4x4 vectors are equal, 2 items
  if they make two equal pairs (upper / lower or left / right), else 4 items; an item's class comes from its vector's fractions:
  0 both zero, 1 yFrac zero, 2 xFrac zero, 4 xFrac 2, 5 yFrac 2 (xFrac odd), 3 both odd;
- per tile, an inter macroblock with any coded bit gives residual items: without the 8x8 transform one per coded luma 4x4 block, with it one 8x8
  item per coded 8x8 block; and one per coded chroma block -- all eight if it has chroma DC;
- the intra kernel walks a row in chunks of 64 macroblocks; an intra macroblock (Intra4x4 / 8x8 / 16x16) waits for the row above if one of the
  three macroblocks above it (left, straight, right) is intra.
"""
import functools
from collections import Counter

import numpy as np

from edge264_amd import backend, packet as P, synth

TILE_W, TILE_H, CHUNK = 16, 4, 64
ALL_I = (P.MB_I4x4, P.MB_I8x8, P.MB_I16x16)


# ---- the census ------------------------------------------------------------------------------------------------------------------------

def mv_class(v) -> int:
    xf, yf = int(v[0]) & 3, int(v[1]) & 3
    if yf == 0:
        return 0 if xf == 0 else 1
    if xf == 0:
        return 2
    if xf == 2:
        return 4
    return 5 if yf == 2 else 3


def quadrant_items(v4) -> list:
    """the classes of the items the four 4x4 vectors (0,0) (4,0) (0,4) (4,4) of a quadrant make"""
    a, b, c, d = (tuple(int(x) for x in v) for v in v4)
    if a == b == c == d:
        return [mv_class(a)]
    if a == b and c == d:
        return [mv_class(a), mv_class(c)]
    if a == c and b == d:
        return [mv_class(a), mv_class(b)]
    return [mv_class(v) for v in (a, b, c, d)]


def _popcount(x) -> int:
    return bin(int(x)).count("1")


def tile_census(pk) -> list:
    """per tile (raster order of tiles): dict(tx, ty, mbs, cnt = [6 item counts of list 0, of list 1], res4 = luma 4x4 residual items,
    chroma = chroma residual items, res8 = 8x8 residual items)"""
    W, H = pk.width_mbs, pk.height_mbs
    mo = pk.motion
    out = []
    for ty in range(0, H, TILE_H):
        for tx in range(0, W, TILE_W):
            t = dict(tx=tx, ty=ty, mbs=0, cnt=[[0] * 6, [0] * 6], res4=0, chroma=0, res8=0)
            for y in range(ty, min(ty + TILE_H, H)):
                for x in range(tx, min(tx + TILE_W, W)):
                    a = y * W + x
                    m = pk.mbs[a]
                    t["mbs"] += 1
                    if int(m["kind"]) != P.MB_INTER or int(m["flags"]) & P.MBF_DONE:
                        continue
                    mv = mo["mvs"][a].reshape(2, 16, 2)
                    for l in (0, 1):
                        for q in range(4):
                            if mo["refPic"][a][l * 4 + q] >= 0:
                                for c in quadrant_items(mv[l, q * 4:q * 4 + 4]):
                                    t["cnt"][l][c] += 1
                    coded = int(m["coded"])
                    if not coded:
                        continue
                    if int(m["flags"]) & P.MBF_T8x8:
                        t["res8"] += _popcount(coded & 0x1111)
                    else:
                        t["res4"] += _popcount(coded & 0xffff)
                    t["chroma"] += 8 if coded & P.CODED_CHROMA_DC else _popcount(coded >> 16 & 255)
            out.append(t)
    return out


def intra_census(pk):
    """(counts, the map of the intra macroblocks this packet reconstructs)"""
    W, H = pk.width_mbs, pk.height_mbs
    kind = pk.mbs["kind"].astype(int).reshape(H, W)
    done = (pk.mbs["flags"].astype(int).reshape(H, W) & P.MBF_DONE) != 0
    intra = np.isin(kind, ALL_I) & ~done
    c = Counter(n_intra=int(intra.sum()), n_pcm=int((kind == P.MB_PCM).sum()), n_inter=int((kind == P.MB_INTER).sum()),
                n_coded_mbs=int(pk.hdr["n_coded_mbs"]), n_inter_mbs=int(pk.hdr["n_inter_mbs"]))

    def at(x, y):
        return 0 <= x < W and 0 <= y < H and bool(intra[y, x])
    row_empty = []
    for y in range(H):
        empty = sum(not intra[y, x0:x0 + CHUNK].any() for x0 in range(0, W, CHUNK))
        row_empty.append(empty)
        c["empty_chunks"] += empty
        c["last_mb_intra"] += int(intra[y, W - 1])
        c["first_mb_intra"] += int(intra[y, 0])
        for x in np.nonzero(intra[y])[0]:
            x = int(x)
            tl, up, tr = at(x - 1, y - 1), at(x, y - 1), at(x + 1, y - 1)
            c["tr_cross"] += int(tr and x % CHUNK == CHUNK - 1)
            c["tl_cross"] += int(tl and x % CHUNK == 0)
            c["only_tr"] += int(tr and not up and not tl)
            c["only_tl"] += int(tl and not up and not tr)
            if y > 0:
                c["below_a_row"] += 1
                # both diagonal neighbours above (where the picture has them) intra, the one straight above not
                c["diagonals_only"] += int(not up and (tl or x == 0) and (tr or x == W - 1))
    c["min_row_empty_chunks"] = min(row_empty)
    return c, intra


def census(pkt) -> dict:
    pk = P.Packet(bytes(pkt))
    counts, intra_map = intra_census(pk)
    return dict(w=pk.width_mbs, h=pk.height_mbs, type={2: "I", 0: "P", 1: "B"}[int(pk.slices[0]["slice_type"])],
                tiles=tile_census(pk) if pk.motion is not None else [], intra=counts, intra_map=intra_map)


# ---- what each case must show, on every P and B picture --------------------------------------------------------------------------------

def _lists(cen):
    return (0, 1) if cen["type"] == "B" else (0,)


def must_one_class(c):
    def check(cen):
        for l in _lists(cen):
            assert any(t["cnt"][l][c] == 1024 and sum(t["cnt"][l]) == 1024 for t in cen["tiles"]), (l, [t["cnt"] for t in cen["tiles"]])
    return check


def must_shared(c):
    def check(cen):
        for l in _lists(cen):
            assert any(t["cnt"][l][c] + t["cnt"][l][5 - c] == 1024 and min(t["cnt"][l][c], t["cnt"][l][5 - c]) >= 256 for t in cen["tiles"]), \
                (l, [t["cnt"] for t in cen["tiles"]])
    return check


def must_all_tiles_full(cen):
    assert any(t["mbs"] == 64 for t in cen["tiles"])
    for l in _lists(cen):
        for t in cen["tiles"]:
            assert sum(t["cnt"][l]) == 16 * t["mbs"], (l, t)  # (1024 in the full tile)
        assert all(t["cnt"][l][c] for t in cen["tiles"] if t["mbs"] == 64 for c in range(6))


def must_res_4x4(cen):
    assert any(t["res4"] + t["chroma"] == 1536 and t["res4"] == 1024 for t in cen["tiles"]), [(t["res4"], t["chroma"]) for t in cen["tiles"]]


def must_res_8x8(cen):
    assert any(t["res8"] == 256 and t["chroma"] == 512 and t["res4"] == 0 for t in cen["tiles"]), [(t["res8"], t["chroma"]) for t in cen["tiles"]]


def must_sat_and_res(cen):
    for l in _lists(cen):
        assert any(sum(t["cnt"][l]) == 1024 and t["res4"] + t["chroma"] == 1536 for t in cen["tiles"])


def must_counts(**least):
    def check(cen):
        assert all(cen["intra"][k] >= v for k, v in least.items()), {k: cen["intra"][k] for k in least}
    return check


def must_columns(cen):
    i = cen["intra"]
    assert i["first_mb_intra"] == cen["h"] and i["last_mb_intra"] == cen["h"], i
    # (64 macroblocks wide: one chunk, whose column 63 is the picture's last -- nothing to cross, and the kernel must not assume there is)
    assert (i["tr_cross"] >= 1 and i["tl_cross"] >= 1) if cen["w"] > CHUNK else i["tr_cross"] + i["tl_cross"] == 0, i


def must_far_ends(cen):
    assert cen["intra"]["min_row_empty_chunks"] >= 2 and cen["intra"]["n_intra"] == 2 * cen["h"], cen["intra"]


def must_lone(key):
    def check(cen):
        assert cen["intra"]["n_intra"] == 1 and cen["intra"][key] == 1, cen["intra"]
    return check


def must_checker(cen):
    i = cen["intra"]
    assert i["n_intra"] == cen["w"] * cen["h"] // 2 and i["below_a_row"] > 0 and i["diagonals_only"] == i["below_a_row"], i


def must_pcm_no_intra(cen):
    i = cen["intra"]
    assert i["n_intra"] == 0 and i["n_pcm"] == 3 and i["n_coded_mbs"] != i["n_inter_mbs"], i


def must_nothing(cen):
    pass


# ---- placements ------------------------------------------------------------------------------------------------------------------------

def placing(pred, other="inter"):
    """place function: "intra" where pred(x, y, W, H), `other` elsewhere"""
    return lambda x, y, W, H: "intra" if pred(x, y, W, H) else other


def mirrored(place):
    return lambda x, y, W, H: place(W - 1 - x, y, W, H)


def _pcm_places(x, y, W, H):
    return "pcm" if (x, y) in ((0, 0), (W - 1, 1), (W // 2, H - 1)) else "inter"


STAIR_RIGHT = placing(lambda x, y, W, H: x == 66 - y or x == W - 1 - y)
STAIR_LEFT = placing(lambda x, y, W, H: x == 61 + y)
COLUMNS = placing(lambda x, y, W, H: x in (0, 63, 64, W - 1))
FAR_ENDS = placing(lambda x, y, W, H: x >= 128 if y & 1 else x < 2)
LONE_LAST = placing(lambda x, y, W, H: (x, y) == (W - 1, H - 1))
LONE_FIRST = placing(lambda x, y, W, H: (x, y) == (0, 0))
CHECKER = placing(lambda x, y, W, H: (x + y) & 1 == 1)

# ---- the cases: (name, [(width, height) in macroblocks], picture types, generator options, check of every P / B picture's census) -------

_SAT = dict(partitions="4x4", both_lists=True, intra_in_inter=0.0)
_PLACED = dict(i_kinds=ALL_I, t8x8=True)
SATURATED = [
    *[(f"sat_one_class_{c}", [(16, 4)], "IPB", dict(_SAT, mv_classes=(c,)), must_one_class(c)) for c in (0, 3, 5)],
    *[(f"sat_shared_{c}{5 - c}", [(16, 4), (32, 8)], "IPB", dict(_SAT, mv_classes=(c, 5 - c)), must_shared(c)) for c in (0, 1, 2)],
    ("sat_all_classes", [(17, 5)], "IPB", dict(_SAT), must_all_tiles_full),
    ("res_full_4x4", [(16, 4), (17, 5)], "IPB", dict(coded_all=True, level_ends=True, intra_in_inter=0.0), must_res_4x4),
    ("res_full_8x8", [(16, 4)], "IPB", dict(coded_all=True, t8x8=True, intra_in_inter=0.0), must_res_8x8),
    ("sat_and_res", [(16, 4)], "IPB", dict(_SAT, coded_all=True, weighted=1), must_sat_and_res),
]
PLACED = [
    ("stair_right", [(130, 5), (130, 19)], "IPB", dict(_PLACED, place=STAIR_RIGHT), must_counts(tr_cross=1, only_tr=3)),
    ("stair_left", [(130, 5), (130, 19)], "IPB", dict(_PLACED, place=STAIR_LEFT), must_counts(tl_cross=1, only_tl=3)),
    ("columns", [(130, 5), (65, 19), (64, 5)], "IPB", dict(_PLACED, place=COLUMNS), must_columns),
    ("far_ends", [(130, 19)], "IPB", dict(_PLACED, place=FAR_ENDS), must_far_ends),
    ("lone_last", [(130, 5), (17, 19)], "IPB", dict(_PLACED, place=LONE_LAST), must_lone("last_mb_intra")),
    ("lone_first", [(130, 5), (17, 19)], "IPB", dict(_PLACED, place=LONE_FIRST), must_lone("first_mb_intra")),
    ("checker", [(33, 19)], "IPB", dict(_PLACED, place=CHECKER), must_checker),
    ("pcm_no_intra", [(20, 5)], "IPB", dict(_PLACED, place=_pcm_places), must_pcm_no_intra),
]
TAIL_WIDTHS, TAIL_HEIGHTS = (3, 4, 5, 8, 9), (7, 8, 9, 15, 16, 17, 30, 31, 32, 33)
TAILS = ("tails", [(w, h) for h in TAIL_HEIGHTS for w in TAIL_WIDTHS], "IPB",
         dict(intra_in_inter=0.2, t8x8=True, i_kinds=ALL_I, residual_prob=0.6), must_nothing)
CASES = {c[0]: c for c in SATURATED + PLACED + [TAILS]}


def seed_of(name, w, h) -> int:
    return 1000 + 97 * list(CASES).index(name) + 7 * w + h


@functools.lru_cache(maxsize=None)
def packets(name, w, h, mirror_second=False):
    """The case's pictures at w x h, generated once per process: [(packet bytes, census)], every packet accepted by the validator and every
    P / B picture's census checked against what the case must show.  mirror_second: picture types I P P, the second P picture's placement
    mirrored left to right."""
    _, geoms, pattern, kw, must = CASES[name]
    assert (w, h) in geoms
    g = synth.StreamSynth(w, h, seed_of(name, w, h), **kw)
    out = []
    for i, t in enumerate("IPP" if mirror_second else pattern):
        if mirror_second and i == 2:
            g.place = mirrored(kw["place"])
        p = bytes(g.next_frame(t))
        assert backend.packet_check(p) == 0, (name, w, h, i, backend.last_error())
        cen = census(p)
        assert cen["type"] == t
        if mirror_second and i == 2:
            assert np.array_equal(cen["intra_map"], out[1][1]["intra_map"][:, ::-1]) and cen["intra"]["n_intra"] + cen["intra"]["n_pcm"] > 0
        elif t != "I":
            must(cen)
        out.append((p, cen))
    return out


def check(name, w, h, mirror_second=False) -> list:
    """the case's packets, each P / B picture's census held against what the case must show (again: the packets are made once per process)"""
    pkts = packets(name, w, h, mirror_second)
    for i, (_, cen) in enumerate(pkts):
        if cen["type"] != "I" and not (mirror_second and i == 2):
            CASES[name][4](cen)
    return [p for p, _ in pkts]
