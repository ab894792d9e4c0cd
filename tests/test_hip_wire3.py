"""Version-7 packets (the third level of the wire form, include/edge264_compact.h: a run of equal plain entries travels as one entry) through every
host-packet entry point of the C-ABI on the MI355X: e264_expand_kernel with its five popcounts, and a repeat reading its source's entry, in front of the four
kernels.  tests/test_hip_wire2.py at level 3, on the pictures with planted runs of tests/run_cases.py.  Expectation: the pictures the version-4 packets give
through the same entry point and, for the front end with e264front_set_compact(3), the unmodified reference's md5s."""
import ctypes as C
import glob
import hashlib
import json
import os

import pytest

from edge264_amd import backend, synth
from tests import run_cases
from tests.test_hip_wire import _gop, run, synth_streams

HERE = os.path.dirname(os.path.abspath(__file__))
STREAMS = os.path.join(HERE, "golden", "streams")
FRONT = os.path.join(os.path.dirname(HERE), "edge264_amd", "libedge264_hipfront.so")
SMALL = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(STREAMS, "*.264")) if os.path.getsize(p) < 60_000)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


def fold3(per_stream):
    return [[backend.packet_fold(p, 3) for p in ps] for ps in per_stream]


def n_repeat(wire):
    """E264CompactHdr3.n_repeat of a version-7 packet"""
    return int.from_bytes(wire[int.from_bytes(wire[40:44], "little") + 20:][:4], "little")


def planted_40(w=7, h=5):
    """40 streams of 7 x 5 macroblocks (>= 32 pinned packets: the gathered transfer), a run planted in every P and B picture"""
    out = []
    for k in range(40):
        g = synth.StreamSynth(w, h, seed=300 + k, p_skip=0.5, residual_prob=0.9, place=lambda x, y, w_, h_: "inter")
        out.append([p if ft == "I" else run_cases.plant(p, [("run", k % h, k % 3, 3 + k % 4)]) for ft, p in ((ft, bytes(g.next_frame(ft))) for ft in "IPBP")])
    return out


@pytest.mark.parametrize("how", ["single", "host", "pinned", "pinned_untrusted", "resident"])
def test_version7_packets_give_the_same_pictures(device, how):
    cases = [per_stream for _, per_stream in run_cases.streams(2)]
    cases.append(planted_40() if how != "single" else planted_40()[:2])
    reps = 0
    for per_stream in cases:
        wire = fold3(per_stream)
        assert all(w[4] == 7 for ws in wire for w in ws)
        reps += sum(n_repeat(w) for ws in wire for w in ws)
        assert run(device, wire, how) == run(device, per_stream, how)
    assert reps > 800


def test_mixed_batches_and_growing_motion_sections(device):
    """one submission with version-4, -5, -6 and -7 packets side by side; a stream whose later pictures need a larger expansion buffer"""
    pics = [p for _, p, _ in run_cases.cases()["20x6"]] + [p for _, p, _ in run_cases.cases()["20x6"]][1:]
    a = [list(pics) for _ in range(8)]
    mixed = [[backend.packet_fold(p, (k + i) % 4) if (k + i) % 4 else p for i, p in enumerate(ps)] for k, ps in enumerate(a)]
    assert {w[4] for ws in mixed for w in ws} == {4, 5, 6, 7}
    assert {ws[1][4] for ws in mixed} == {4, 5, 6, 7}  # (in ONE submission)
    assert run(device, mixed, "host") == run(device, a, "host")
    g = synth.StreamSynth(20, 6, seed=9, p_skip=0.95, residual_prob=0.9, place=lambda x, y, w, h: "inter")
    first = [p if i == 0 else run_cases.plant(p, [("run", 1, 0, 19), ("run", 4, 3, 17)]) for i, p in enumerate(_gop(g, "IPP"))]
    g.p_skip = 0.3  # many partitioned macroblocks: longer motion records
    later = _gop(g, "PBPB")
    grow = [first + later]
    wire = fold3(grow)
    assert sum(n_repeat(w) for w in wire[0]) > 60
    assert run(device, wire, "single") == run(device, grow, "single")


@pytest.fixture(scope="module")
def _hipfront_lib():
    if not os.path.exists(FRONT):
        pytest.fail(f"{FRONT} missing: it is built in the container by `make -C oracle ref` and travels with the snapshot")
    from oracle.pyoracle import HipFront
    h = HipFront()
    h.lib.e264front_set_compact.argtypes = [C.c_int]
    return h


@pytest.fixture
def hipfront(_hipfront_lib):
    """the front library on the device sink, folding at level 3 (both switches are global to the library: set per test, and set back)"""
    _hipfront_lib.lib.e264front_set_sink(0)
    _hipfront_lib.lib.e264front_set_compact(3)
    yield _hipfront_lib
    _hipfront_lib.lib.e264front_set_compact(0)


@pytest.mark.parametrize("name", SMALL)
def test_front_end_at_level3_matches_reference(name, hipfront):
    """the small committed streams through edge264.h on the device sink with the front end folding its packets at level 3: the unmodified reference's
    frames and codes"""
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    data = open(os.path.join(STREAMS, name + ".264"), "rb").read()
    frames, codes = hipfront.decode(data)
    assert codes == sums[name]["nal_codes"]
    assert [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames] == sums[name]["md5"]


def test_concealment_at_level3(hipfront):
    """three damaged-stream scenarios with the front end folding at level 3: pictures that leave in several packets (their records edited in the packet
    before the fold) through the device expansion -- the unmodified reference's frames"""
    from tests import damage
    with open(os.path.join(STREAMS, "damage_md5.json")) as f:
        sums = json.load(f)
    for name, which, keep in damage.RESENT[:3]:
        frames, codes = hipfront.decode(damage.truncated_then_resent(name, which, keep))
        want = sums[f"{name}-{which}-{keep}"]
        assert codes == want["nal_codes"], (name, which, keep)
        assert [hashlib.md5(b"".join(p.tobytes() for p in fr)).hexdigest() for fr in frames] == want["md5"], (name, which, keep)


def test_multi_stream_driver_at_level3(tmp_path):
    """e264_multi (decoders on parser threads, packets in page-locked memory submitted in place and trusted) with E264_FRONT_COMPACT=3: the reference's frames"""
    import subprocess
    root = os.path.dirname(HERE)
    exe, hip = os.path.join(root, "edge264_amd", "e264_multi"), os.path.join(root, "edge264_amd", "libedge264_hip.so")
    for p in (exe, FRONT, hip):
        assert os.path.exists(p), f"{p} missing (built by __graft_entry__.build())"
    with open(os.path.join(STREAMS, "reference_md5.json")) as f:
        sums = json.load(f)
    names = ["nat_small_ipp8", "cabac_nat_small_ibbp10"]
    files = [os.path.join(STREAMS, n + ".264") for n in names]
    out = subprocess.run([exe, "--front", FRONT, "--hip", hip, "--threads", "2", "--out", str(tmp_path)] + files,
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, E264_FRONT_COMPACT="3"))
    assert out.returncode == 0, out.stderr[-2000:]
    stats = json.loads(out.stdout.strip().splitlines()[-1])
    assert stats["frames"] == sum(len(sums[n]["md5"]) for n in names)
    for k, n in enumerate(names):
        nby = sums[n]["width_mbs"] * 16 * sums[n]["height_mbs"] * 16 * 3 // 2 * sums[n]["views"]
        data = open(tmp_path / f"s{k}.yuv", "rb").read()
        assert [hashlib.md5(data[i:i + nby]).hexdigest() for i in range(0, len(data), nby)] == sums[n]["md5"], f"stream {k} ({n})"
