"""The prediction kernel's one-trip phases on the MI355X against the oracle: the 17 x 5 pictures of tests/pred_fetch_cases.py (every shape of motion record
beside every other, quadrants one list does not predict, the records that END the motion section, and the macroblocks whose payload is the packet's last
bytes or its first: chroma DC alone, a 4x4 and an 8x8 luma block in byte form, chroma AC without chroma DC, I_PCM) as resident packets -- which sit in
allocations of exactly their size -- through all four kernels, every stream once alone and once in a batch of eight streams.  Every picture must equal the
oracle's.  tests/test_pred_fetch_emu.py runs the same packets through the kernel's source on the host, under the sanitizers too."""
import pytest

from edge264_amd import backend
from tests import pred_fetch_cases as F
from tests.test_hip_forms import decoders, options, run_batch

pytestmark = pytest.mark.gpu
BATCH = 8


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def cases():
    out = F.streams()
    for name, pkts in out.items():
        assert len(pkts) == 3 and all(backend.packet_check(p) == 0 for p in pkts), name
    return out


def test_alone(device, oracle, cases):
    for name, pkts in cases.items():
        with options(device) as cfg, decoders(device, 1) as decs:
            for ft, pkt in zip("IPB", pkts):
                f = run_batch(device, oracle, "resident", decs, [pkt], cfg, label=f"{name} {ft} alone")
                assert (f.get("pred", 0) == 1) == (ft != "I"), (name, ft, f)


def test_batches_of_eight(device, oracle, cases):
    names = list(cases)
    names += names[:-len(names) % BATCH]  # (the last batch is filled up with the first streams again)
    for k in range(0, len(names), BATCH):
        group = names[k:k + BATCH]
        with options(device) as cfg, decoders(device, BATCH) as decs:
            for i, ft in enumerate("IPB"):
                f = run_batch(device, oracle, "resident", decs, [cases[n][i] for n in group], cfg, label=f"{'+'.join(group)} {ft}")
                assert f.get("pred", 0) == (BATCH if ft != "I" else 0), (group, ft, f)
