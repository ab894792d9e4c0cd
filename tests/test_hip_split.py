"""The kernels on the MI355X on pictures that arrive in several packets (tests/split_cases.py): E264_MBF_DONE records beside fresh ones inside a tile,
across the intra kernel's chunk boundary and across the deblocking kernel's row groups, macroblocks deblocked by a later packet than the one that
reconstructed them, packets without a fresh macroblock.  tests/test_split_emu.py runs the same packets through the kernels' source on the host, where
the waves run one after another; an intra row that waits for a DONE macroblock or does not wait for a fresh one, a bitmap word that holds a DONE
macroblock, a bitmap left over for the next packet show here only.

Every packet's whole slot is compared with Oracle.decode_frame, every submission's launch counts with the rule table of tests/test_hip_forms.py, every
case's census with its minimum where the packets are made.  The packets of a case are made once per process."""
import functools
from collections import Counter

import numpy as np
import pytest

from edge264_amd import backend, packet as P, synth
from tests import split_cases as S
from tests.test_hip_forms import REACHES, SETTINGS, decoders, options, run_batch

pytestmark = pytest.mark.gpu
CASES = [(shape, w, h) for shape in S.SHAPES for (w, h) in S.GEOMS]
IDS = [f"{s}_{w}x{h}" for s, w, h in CASES]
SPLIT_SETTINGS = ["defaults", "split_planes0", "waves8", "waves2", "intra_waves8", "intra_waves4"]


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


@functools.lru_cache(maxsize=None)
def companions():
    """a 5 x 4 and a 1 x 9 random stream, one picture for every packet of the longest case"""
    return [synth.StreamSynth(w, h, 180 + k, t8x8=True, i_kinds=S.ALL_I, intra_in_inter=0.2).gop("IPBP" * 10) for k, (w, h) in enumerate(((5, 4), (1, 9)))]


def alone_and_in_a_submission(dev, oracle, cfg, shape, stream, w, h, label):
    """the stream's packets on one decoder alone, and on another in resident submissions beside the two companions"""
    pkts, names = S.flat(S.packets(shape, stream, w, h))
    side = companions()
    total = Counter()
    with decoders(dev, 4) as (alone, d0, d1, d2):
        for i, (p, n) in enumerate(zip(pkts, names)):
            total.update(run_batch(dev, oracle, "single", [alone], [p], cfg, label=f"{label} packet {n} alone"))
            total.update(run_batch(dev, oracle, "resident", [d0, d1, d2], [p, side[0][i], side[1][i]], cfg, label=f"{label} packet {n} of a submission"))
    return total


@pytest.mark.parametrize("setting", SPLIT_SETTINGS)
@pytest.mark.parametrize("shape,w,h", CASES, ids=IDS)
def test_split_pictures(device, oracle, shape, w, h, setting):
    """every shape at every geometry, both base streams, the whole slot after every packet"""
    total = Counter()
    with options(device, **SETTINGS[setting]) as cfg:
        for stream in S.STREAMS:
            total.update(alone_and_in_a_submission(device, oracle, cfg, shape, stream, w, h, f"{shape} {stream} {w}x{h} {setting}"))
    assert sum(total[f] for f in REACHES[setting]) > 0, total
    assert total["pred"] > 0 and total[f"intra{cfg['intra_waves']}_bitmap"] > 0, total


# ---- splits that must not show ---------------------------------------------------------------------------------------------------------------------

def held_against_the_unsplit_packet(dev, oracle, cfg, stream, w, h, deblock, split_types, label):
    """One decoder takes the stream's unsplit packets, one decoder per cut set the split ones (the k-th packets of all of them in one resident
    submission): after a picture's last packet every slot equals the first decoder's, byte for byte."""
    sets = S.cut_sets(w, h)
    with decoders(dev, 1 + len(sets)) as (whole, *parts):
        for i, (t, raw) in enumerate(zip(S.PATTERN, S.base(stream, w, h, deblock=deblock))):
            run_batch(dev, oracle, "single", [whole], [raw], cfg, label=f"{label} picture {i}{t} unsplit")
            per = [S.raster_split(raw, w, h, cuts) if t in split_types else [raw] for cuts in sets]
            for k in range(max(len(p) for p in per)):
                sel = [(d, p[k]) for d, p in zip(parts, per) if k < len(p)]
                run_batch(dev, oracle, "resident", [d for d, _ in sel], [p for _, p in sel], cfg, label=f"{label} picture {i}{t} packets {k}")
            slot = int(P.Packet(raw).hdr["dst_slot"])
            want = whole.st.download(slot)
            for cuts, d in zip(sets, parts):
                got = d.st.download(slot)
                assert np.array_equal(got, want), f"{label} picture {i}{t} cut at {cuts}: {int((got != want).sum())} bytes differ from the unsplit packet's picture, the first at {int(np.argmax(got != want))}"


@pytest.mark.parametrize("w,h", S.GEOMS, ids=[f"{w}x{h}" for w, h in S.GEOMS])
def test_raster_split_without_deblocking_is_invisible(device, oracle, w, h):
    """the rich stream without deblocking, every picture in two and three packets (tests/test_split_emu.py says why the split cannot show)"""
    with options(device) as cfg:
        held_against_the_unsplit_packet(device, oracle, cfg, "rich", w, h, False, "IPB", f"no deblocking {w}x{h}")


@pytest.mark.parametrize("w,h", S.GEOMS, ids=[f"{w}x{h}" for w, h in S.GEOMS])
def test_raster_split_of_inter_pictures_is_invisible(device, oracle, w, h):
    """the inter stream with deblocking, its P and B pictures in two and three packets"""
    with options(device) as cfg:
        held_against_the_unsplit_packet(device, oracle, cfg, "inter", w, h, True, "PB", f"inter stream {w}x{h}")


# ---- a packet with nothing to reconstruct, split off to the second queue ----------------------------------------------------------------------------

@pytest.mark.parametrize("setting", ["defaults", "split_planes0"])
@pytest.mark.parametrize("w,h", [(17, 5), (66, 9)], ids=["17x5", "66x9"])
def test_deblock_only_packet_beside_a_p_picture(device, oracle, w, h, setting):
    """An I picture without I_PCM whose second packet holds DONE records and deblocking alone, beside a P picture of another stream: the packet has
    no prediction work, so its intra pass is split off to the second queue -- with nothing to reconstruct.  The P picture that follows on the same
    decoder (intra macroblocks among its inter ones, again in two packets) must find no bitmap left over."""
    g = synth.StreamSynth(w, h, S.seed_of("rich", w, h) + 1, **dict(S.STREAMS["rich"], pcm_prob=0.0))
    n_packets, r, delay = S.late_deblock(w, h)
    mine = [p for t in "IPP" for p in S.split(bytes(g.next_frame(t)), r, n_packets, delay)]
    cens = [S.census(p) for p in mine]
    assert [c["fresh"] for c in cens] == [w * h, 0] * 3 and [c["done_deblocked"] for c in cens] == [0, w * h] * 3
    assert cens[0]["fresh_intra"] == w * h and cens[2]["fresh_intra"] > 0 and cens[2]["fresh_inter"] > 0 and not any(c["done_pcm"] for c in cens)
    other = companions()[0]  # I P B P ...
    with options(device, **SETTINGS[setting]) as cfg, decoders(device, 2) as decs:
        for i, p in enumerate(mine):
            f = run_batch(device, oracle, "resident", decs, [p, other[i]], cfg, label=f"deblock-only {w}x{h} {setting} packet {i}")
            if i == 1:
                assert f.get("intra_split", 0) + f.get("intra_planes_split", 0) == 1 and f["pred"] == 1, f
            if i == 2:
                assert f["pred"] == 2 and f["intra16_bitmap"] == 2, f


# ---- the wire form ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["host", "pinned"])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("shape,w,h", [("hole", 66, 9), ("checker", 17, 5)], ids=["hole_66x9", "checker_17x5"])
def test_split_pictures_in_wire_form(device, oracle, shape, w, h, level, how):
    """two cases as wire packets of both levels: the expansion kernel in front of the same records (a DONE record stays a full record)"""
    side = companions()
    with options(device) as cfg, decoders(device, 3) as decs:
        for stream in S.STREAMS:
            pkts, names = S.flat(S.packets(shape, stream, w, h))
            for i, (p, n) in enumerate(zip(pkts, names)):
                v4s = [p, side[0][i], side[1][i]]
                wire = [backend.packet_compact(q, level=level) for q in v4s]
                assert all(q[4] == 4 + level and backend.packet_check(q) == 0 for q in wire)
                f = run_batch(device, oracle, how, decs, v4s, cfg, sent=wire, label=f"{shape} {stream} {w}x{h} level {level} packet {n}")
                assert f["expand"] == 3, f
