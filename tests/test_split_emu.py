"""Pictures sent in several packets (tests/split_cases.py) on the CPU: the kernels' source built for the host (tests/emu) against the oracle after
every packet, every variant of tests/test_layouts_emu.py on the tight layout and one padded layout on one variant; two checks that do not rest on the
oracle's own reading of E264_MBF_DONE (a split that must leave the picture as the unsplit packet leaves it), on the oracle and on the emulation; the
wire form of the split packets.  The census of every case is asserted where its packets are made (split_cases.packets).  The host build runs the
waves one after another: a wait that is missing or a bitmap word left over shows on the device only (tests/test_hip_split.py)."""
import numpy as np
import pytest

from edge264_amd import backend, packet as P
from tests import layouts as L, split_cases as S
from tests.test_layouts_emu import N_SLOTS, VARIANTS, libs, run_case, run_pipeline  # noqa: F401 (libs: the fixture)

CASES = [(shape, w, h) for shape in S.SHAPES for (w, h) in S.GEOMS]
IDS = [f"{s}_{w}x{h}" for s, w, h in CASES]


def run(libs, oracle, variant, layout, shape, w, h):
    for stream in S.STREAMS:
        pkts, labels = S.flat(S.packets(shape, stream, w, h))
        run_case(libs, variant, layout, w, h, labels, {}, S.seed_of(stream, w, h), oracle=oracle, name=f"{shape} {stream}", packets=pkts)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape,w,h", CASES, ids=IDS)
def test_split_emu_vs_oracle(libs, oracle, shape, w, h, variant):
    run(libs, oracle, variant, "tight", shape, w, h)


@pytest.mark.parametrize("shape,w,h", CASES, ids=IDS)
def test_split_on_a_padded_layout(libs, oracle, shape, w, h):
    run(libs, oracle, list(VARIANTS)[(len(shape) + h) % len(VARIANTS)], "pad16", shape, w, h)


# ---- splits that must not show ---------------------------------------------------------------------------------------------------------------------

def held_against_the_unsplit_packet(decode, stream, w, h, deblock, split_types, label, part=(0, 1)):
    """decode(packet, slots): every picture of the stream whose type is in split_types, split at every cut set (part = (k, m): at every m-th,
    starting with the k-th), leaves its slot byte for byte as its unsplit packet does -- from the same slots before it"""
    raws = S.base(stream, w, h, deblock=deblock)
    hdr = L.hdr_of(raws[0])
    rng = np.random.default_rng(S.seed_of(stream, w, h))
    dpb = [L.random_slot(hdr, rng) for _ in range(N_SLOTS)] + [None] * (P.MAX_SLOTS - N_SLOTS)
    sets = S.cut_sets(w, h)[part[0]::part[1]]
    n = 0
    for i, (t, raw) in enumerate(zip(S.PATTERN, raws)):
        d = int(P.Packet(raw).hdr["dst_slot"])
        before = [None if a is None else a.copy() for a in dpb]
        decode(raw, dpb)
        for cuts in sets if t in split_types else []:
            mine = [None if a is None else a.copy() for a in before]
            for p in S.raster_split(raw, w, h, cuts):
                decode(p, mine)
            assert np.array_equal(mine[d], dpb[d]), L.first_difference(hdr, mine[d], dpb[d], f"{label} {stream} {w}x{h} picture {i}{t} cut at {cuts}")
            n += 1
    assert n == len(sets) * sum(t in split_types for t in S.PATTERN) > 0


def emu_decoders(libs):
    """the pipeline of a submission in two variants, each on every second cut set: version-4 packets, scan form; wire packets, bitmap form"""
    return [(v, lambda p, dpb, v=v: run_pipeline(libs, v, p, dpb), (k, 2)) for k, v in enumerate(("product_scan_mixed_v4", "gs2_bitmap_mixed_wire"))]


@pytest.mark.parametrize("w,h", S.GEOMS, ids=[f"{w}x{h}" for w, h in S.GEOMS])
def test_raster_split_without_deblocking_is_invisible(libs, oracle, w, h):
    """No deblocking: a macroblock's samples are final once it is reconstructed, and a later one reads them the same whichever packet wrote them.
    The rich stream, I, P and B pictures, in two and three packets."""
    held_against_the_unsplit_packet(lambda p, dpb: oracle.decode_frame(p, dpb, 3), "rich", w, h, False, "IPB", "oracle")
    for name, decode, part in emu_decoders(libs):
        held_against_the_unsplit_packet(decode, "rich", w, h, False, "IPB", name, part)


@pytest.mark.parametrize("w,h", S.GEOMS, ids=[f"{w}x{h}" for w, h in S.GEOMS])
def test_raster_split_of_inter_pictures_is_invisible(libs, oracle, w, h):
    """Deblocking on, FilterOffsetA / B 4 / -2, I_PCM among the inter macroblocks: nothing of a P or B picture of the inter stream reads the picture's
    own samples before it is deblocked, and the deblocking of a raster prefix touches that prefix alone, in the order of the unsplit packet.  (Its I
    picture goes unsplit: intra prediction behind the cut would read deblocked samples.)"""
    held_against_the_unsplit_packet(lambda p, dpb: oracle.decode_frame(p, dpb, 3), "inter", w, h, True, "PB", "oracle")
    for name, decode, part in emu_decoders(libs):
        held_against_the_unsplit_packet(decode, "inter", w, h, True, "PB", name, part)


# ---- the wire form ---------------------------------------------------------------------------------------------------------------------------------

def compact_bits(wire) -> np.ndarray:
    """H x W: the macroblock is a compact entry (include/edge264_compact.h: the first bitmap behind the header and the three numbers per row)"""
    h = np.frombuffer(wire, P.FRAME_HDR, 1)[0]
    wm, hm, base = int(h["width_mbs"]), int(h["height_mbs"]), int(h["mbs_off"])
    level = {P.E264_VERSION_COMPACT: 1, P.E264_VERSION_COMPACT2: 2}[int(h["version"])]
    wpr = int(np.frombuffer(wire, "<u4", 4, base)[3])
    assert wpr == (wm + 31) // 32
    words = np.frombuffer(wire, "<u4", hm * wpr, base + (16, 24)[level - 1] + 12 * hm).reshape(hm, wpr)
    return np.array([[int(words[y, x >> 5]) >> (x & 31) & 1 for x in range(wm)] for y in range(hm)], bool)


def round_trip(p, wire, level, label):
    """The expansion of the wire packet says what the packet says, and folding it again gives the wire bytes.  It is the CANONICAL version-4 packet
    (include/edge264_compact.h): its motion section holds the records of its inter macroblocks alone -- what the records of ABSENT macroblocks have
    orphaned is gone -- and payload_off travels where a record has residual.  A packet of a picture without a motion section has nothing of either
    kind: it comes back byte for byte."""
    back = backend.packet_expand(wire)
    assert backend.packet_check(back) == 0, (label, backend.last_error())
    assert backend.packet_compact(back, level=level) == wire, label
    a, b = P.Packet(p), P.Packet(back)
    for f in ("kind", "flags", "qp", "chroma_mode", "i16_mode", "nz_mask", "slice", "coded", "dbk_slice"):
        assert np.array_equal(a.mbs[f], b.mbs[f]), (label, f)
    own = (a.mbs["coded"] != 0) | ((a.mbs["kind"] == P.MB_PCM) & ((a.mbs["flags"] & P.MBF_DONE) == 0))
    assert np.array_equal(a.mbs["payload_off"][own], b.mbs["payload_off"][own]), label
    intra = np.isin(a.mbs["kind"], S.ALL_I)
    assert np.array_equal(a.mbs["modes"][intra], b.mbs["modes"][intra]), label
    if int(a.hdr["n_inter_mbs"]):  # (a packet whose inter macroblocks are all still ABSENT comes back without its motion section)
        assert a.motion.tobytes() == b.motion.tobytes(), label
    else:
        assert b.motion is None, label
    assert a.slices.tobytes() == b.slices.tobytes(), label
    assert bytes(a.data[a.payload_off:a.payload_off + int(a.hdr["payload_bytes"])]) == bytes(b.data[b.payload_off:b.payload_off + int(b.hdr["payload_bytes"])]), label
    if not int(a.hdr["motion_off"]):
        assert back == p, label


@pytest.mark.parametrize("shape,w,h", CASES, ids=IDS)
def test_split_packets_fold_and_unfold(shape, w, h):
    """every split packet folds at levels 1 and 2 and comes back from the fold (round_trip); a DONE record never folds (tests/test_compact2.py says so
    for entries), a record that is neither DONE nor ABSENT folds as in the unsplit packet"""
    folded = done = 0
    for stream in S.STREAMS:
        for raw, pkts in zip(S.base(stream, w, h), S.packets(shape, stream, w, h)):
            whole = {level: compact_bits(backend.packet_compact(raw, level=level)) for level in (1, 2)}
            for p in pkts:
                pk = P.Packet(p)
                flags = pk.mbs["flags"].astype(int).reshape(h, w)
                is_done, fresh = (flags & P.MBF_DONE) != 0, ((flags & P.MBF_DONE) == 0) & (pk.mbs["kind"].reshape(h, w) != P.MB_ABSENT)
                for level in (1, 2):
                    wire = backend.packet_compact(p, level=level)
                    assert wire[4] == 4 + level and backend.packet_check(wire) == 0, (stream, level, backend.last_error())
                    round_trip(p, wire, level, (shape, stream, w, h, level))
                    bits = compact_bits(wire)
                    assert not bits[is_done].any() and np.array_equal(bits[fresh], whole[level][fresh]), (shape, stream, w, h, level)
                    folded += int(bits.sum())
                done += int(is_done.sum())
    assert folded > 0 and done > 0
