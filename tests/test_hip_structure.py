"""The kernels on the MI355X on pictures whose structure reaches a capacity or a hand-off boundary inside a kernel (tests/structure_cases.py):
class lists of the prediction kernel filled to the last slot and two classes meeting inside the array they share, full residual lists, intra
macroblocks placed where the intra kernel's wavefront crosses a 64-macroblock chunk or finds chunks and rows empty, picture heights around the
deblocking kernel's row groups.  tests/test_structure_emu.py runs the same packets through the kernels' source on the host, where the waves
run one after another; an intra row that does not wait, a progress value published too early, two tiles racing on bitmap words show here only.

Every picture's whole slot is compared with Oracle.decode_frame, every submission's launch counts with the rule table of
tests/test_hip_forms.py, every P / B picture's census with what its case must show.  The packets of a case are made once per process."""
import functools
from collections import Counter

import pytest

from edge264_amd import backend, synth
from tests import structure_cases as S
from tests.test_hip_forms import REACHES, SETTINGS, _wire_layout, decoders, options, run_batch

pytestmark = pytest.mark.gpu
SAT_GEOMS = [(c[0], w, h) for c in S.SATURATED for (w, h) in c[1]]
PLACED_GEOMS = [(c[0], w, h) for c in S.PLACED for (w, h) in c[1]]
PLACED_SETTINGS = ["defaults", "split_planes0", "intra_waves8", "intra_waves4"]
TAIL_SETTINGS = ["defaults", "split_planes0", "waves107", "waves8", "waves2"]
# the tails' fifty geometries three per submission, heights and widths mixed
TAIL_GROUPS = [(S.TAILS[1][k::17] + S.TAILS[1][:1])[:3] for k in range(17)]


def ids(geoms):
    return [f"{n}_{w}x{h}" for n, w, h in geoms]


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


@functools.lru_cache(maxsize=None)
def companions(pattern):
    """a 5 x 4 and a 1 x 9 random stream beside the case's picture in a submission: max_tiles and max_mbs exceed the small pictures"""
    return [synth.StreamSynth(w, h, 80 + k, t8x8=True, i_kinds=S.ALL_I, intra_in_inter=0.2).gop(pattern) for k, (w, h) in enumerate(((5, 4), (1, 9)))]


def alone_and_in_a_submission(dev, oracle, cfg, name, w, h, label):
    """the case's pictures on one decoder alone, and on another in one resident submission with the two companions"""
    pkts = S.check(name, w, h)
    side = companions(S.CASES[name][2])
    total = Counter()
    with decoders(dev, 4) as (alone, d0, d1, d2):
        for i, p in enumerate(pkts):
            total.update(run_batch(dev, oracle, "single", [alone], [p], cfg, label=f"{label} picture {i} alone"))
            total.update(run_batch(dev, oracle, "resident", [d0, d1, d2], [p, side[0][i], side[1][i]], cfg, label=f"{label} picture {i} of a submission"))
    return total


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name,w,h", SAT_GEOMS, ids=ids(SAT_GEOMS))
def test_saturated_lists(device, oracle, name, w, h, setting):
    """1024 items in one class list, two classes sharing one array to its last slot, 1536 residual items in a tile, under every setting"""
    with options(device, **SETTINGS[setting]) as cfg:
        total = alone_and_in_a_submission(device, oracle, cfg, name, w, h, f"{name} {w}x{h} {setting}")
    assert sum(total[f] for f in REACHES[setting]) > 0, total
    assert total["pred"] > 0, total


@pytest.mark.parametrize("setting", PLACED_SETTINGS)
@pytest.mark.parametrize("name,w,h", PLACED_GEOMS, ids=ids(PLACED_GEOMS))
def test_placed_intra(device, oracle, name, w, h, setting):
    """intra macroblocks on both sides of a chunk boundary, in the first and last column, alone in the picture, in a checkerboard; 19 rows
    for 16, 8 or 4 waves"""
    with options(device, **SETTINGS[setting]) as cfg:
        total = alone_and_in_a_submission(device, oracle, cfg, name, w, h, f"{name} {w}x{h} {setting}")
    assert sum(total[f] for f in REACHES[setting]) > 0, total
    assert total[f"intra{cfg['intra_waves']}_bitmap"] > 0, total


@functools.lru_cache(maxsize=None)
def other_stream_i_pictures():
    return synth.StreamSynth(9, 6, 90, t8x8=True, i_kinds=S.ALL_I).gop("III")


@pytest.mark.parametrize("setting", ["defaults", "split_planes0"])
@pytest.mark.parametrize("name,w,h", PLACED_GEOMS, ids=ids(PLACED_GEOMS))
def test_placed_intra_beside_a_split_off_i_picture(device, oracle, name, w, h, setting):
    """The placed P picture beside an I picture of another stream: that one's intra pass is split off to the second queue and runs while the
    placed picture's prediction kernel writes its bitmap.  Then a second P picture on the same decoder with the placement mirrored left to
    right: a bitmap left over from the picture before would show."""
    pkts = S.check(name, w, h, mirror_second=True)
    others = other_stream_i_pictures()
    with options(device, **SETTINGS[setting]) as cfg, decoders(device, 2) as decs:
        for i, (p, o) in enumerate(zip(pkts, others)):
            f = run_batch(device, oracle, "resident", decs, [p, o], cfg, label=f"{name} {w}x{h} {setting} picture {i} beside an I picture")
            if i:
                assert f.get("intra_split", 0) + f.get("intra_planes_split", 0) == 1 and f["pred"] == 1 and f["intra16_bitmap"] == 1, f


@pytest.mark.parametrize("how", ["host", "pinned"])
@pytest.mark.parametrize("name,w,h", [("stair_right", 130, 5), ("sat_all_classes", 17, 5)], ids=["stair_right_130x5", "sat_all_classes_17x5"])
def test_structure_in_wire_form(device, oracle, name, w, h, how):
    """a placement case and a saturated case as wire packets: the expansion kernel in front of the same lists and the same wavefront"""
    pkts = S.check(name, w, h)
    side = companions(S.CASES[name][2])
    folded = 0
    with options(device) as cfg, decoders(device, 3) as decs:
        for i, p in enumerate(pkts):
            v4s = [p, side[0][i], side[1][i]]
            wire = [backend.packet_compact(q) for q in v4s]
            assert all(backend.packet_check(q) == 0 for q in wire)
            n_compact = _wire_layout(wire[0])[1]
            if name.startswith("sat_"):
                assert n_compact == 0, (i, n_compact)  # four different vectors in every quadrant: nothing folds
            folded += n_compact
            f = run_batch(device, oracle, how, decs, v4s, cfg, sent=wire, label=f"{name} {w}x{h} wire picture {i}")
            assert f["expand"] == 3, f
    assert (folded > 0) == (name == "stair_right"), folded


@pytest.mark.parametrize("setting", TAIL_SETTINGS)
@pytest.mark.parametrize("group", range(len(TAIL_GROUPS)))
def test_tail_heights(device, oracle, group, setting):
    """heights 7 .. 33 macroblocks: chroma heights that are whole deblocking groups (15, 30), tails of one row (16, 31), a luma tail of one row beside
    a full chroma group (17, 33); three geometries per submission"""
    geoms = TAIL_GROUPS[group]
    streams = [S.check("tails", w, h) for w, h in geoms]
    total = Counter()
    with options(device, **SETTINGS[setting]) as cfg, decoders(device, len(geoms)) as decs:
        for i in range(len(streams[0])):
            total.update(run_batch(device, oracle, "resident", decs, [s[i] for s in streams], cfg, label=f"tails {geoms} {setting} picture {i}"))
    assert sum(total[f] for f in REACHES[setting]) > 0, total
