"""The parameter kernel's one-trip motion fetch on the MI355X against the oracle: the pictures of tests/motion_fetch_cases.py (every shape of motion record
beside every other, quadrants one list does not predict, the records that END the motion section and with it the packet; a quadrant NO list predicts has
parameters but no defined samples: that one stays with the host tests -- so the P pictures here, which have list 0 alone, have no unused quadrant at all, and
the case reaches the device through the B pictures, one list at a time) as resident packets -- which sit in
allocations of exactly their size -- and in wire form, as I, P and B pictures.  A size's cases are the streams of one submission, beside an ordinary picture
of another size: with that one in step the P pictures take e264_dbkparam2_kernel<false>, with a B picture beside them the <true> form.
tests/test_motion_fetch_emu.py runs the same packets through the kernel's source on the host, under the sanitizers too."""
import pytest

from edge264_amd import backend, packet as P, synth
from tests import motion_fetch_cases as M
from tests.test_hip_forms import decoders, options, run_batch

pytestmark = pytest.mark.gpu
SIZE_IDS = [f"{w}x{h}" for w, h in M.SIZES]


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def streams(w, h):
    """{case: its I, P, B packets}"""
    out = {}
    for name, ft, pkt in M.pictures(w, h, decodable=True):
        assert backend.packet_check(pkt) == 0, (name, ft)
        out.setdefault(name, []).append(pkt)
    return out


def ordinary(ahead):
    """an ordinary stream's three pictures: I P B, or (ahead) the B B P that follow an I and a P nobody decodes (their slots read as zero on both sides)"""
    g = synth.StreamSynth(5, 4, 77, t8x8=True, num_refs=2)
    if ahead:
        g.gop("IP")
    return [bytes(p) for p in g.gop("BBP" if ahead else "IPB")]


@pytest.mark.parametrize("beside", ["in_step", "b_beside_p"])
@pytest.mark.parametrize("w,h", M.SIZES, ids=SIZE_IDS)
def test_resident(device, oracle, w, h, beside):
    cases = streams(w, h)
    other = ordinary(beside == "b_beside_p")
    forms = []
    with options(device) as cfg, decoders(device, len(cases) + 1) as decs:
        for i, ft in enumerate("IPB"):
            forms.append(run_batch(device, oracle, "resident", decs, [c[i] for c in cases.values()] + [other[i]], cfg, label=f"{w}x{h} {beside} {ft}"))
    # the form each leg is there for: P (and I) pictures alone take <false> (dbkp_small); with list-1 motion anywhere in the batch everybody takes <true>
    want = ["dbkp_small", "dbkp_small", "dbkp_general"] if beside == "in_step" else ["dbkp_general"] * 3
    for ft, got, form in zip("IPB", forms, want):
        other_form = "dbkp_small" if form == "dbkp_general" else "dbkp_general"
        assert got.get(form) == len(cases) + 1 and other_form not in got, f"{w}x{h} {beside} {ft}: {got}"


@pytest.mark.parametrize("how", ["resident", "host"])
@pytest.mark.parametrize("w,h", M.SIZES, ids=SIZE_IDS)
def test_wire_form(device, oracle, w, h, how):
    cases = streams(w, h)
    other = ordinary(False)
    folded = 0
    with options(device) as cfg, decoders(device, len(cases) + 1) as decs:
        for i, ft in enumerate("IPB"):
            v4s = [c[i] for c in cases.values()] + [other[i]]
            wire = [backend.packet_compact(p) for p in v4s]
            assert all(backend.packet_check(wp) == 0 for wp in wire)
            folded += sum(wp[4] == P.E264_VERSION_COMPACT for wp in wire)
            run_batch(device, oracle, how, decs, v4s, cfg, sent=wire, label=f"{w}x{h} wire {ft}")
    assert folded > 0
