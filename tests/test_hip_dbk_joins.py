"""Both sides of every join of the deblocking filter's edges in one walk, on the MI355X against the oracle.

dk_edge (edge264_amd/csrc/e264_dbk.h) leaves an edge alone for the whole wave when no lane filters it, runs the bS < 4 filter when one does and
the bS 4 filter on top when one needs it; what the three paths hand to the code behind their join changed in round 7.
The pictures here make one walk take all of them: 24 x 9 macroblocks -- two luma groups (8 rows + a tail of one) and one chroma group -- whose
P pictures are, in the left 12 columns, 16x16 macroblocks without residual on one zero vector into one reference (every bS 0: the steps 7 .. 11
of the first luma group and 8 .. 11 of the chroma group hold nothing but such macroblocks, every edge of theirs takes the wave-wide early-out)
and intra macroblocks in the right 12 columns (bS 3 inside, bS 4 on macroblock edges: the strong filter).  FilterOffsetA = +6 and
FilterOffsetB = -6 put alpha at ~20 and beta at ~3 around QP 28, so that many lines pass the alpha test and fail a beta test: lanes of one
wave disagree about an edge.

The census (CPU) holds the packets to all of that from the oracle's boundary strengths and its unfiltered reconstruction, and runs them through
the kernel's source on the host (tests/emu); the GPU tests run them on the one-workgroup form and on the two-workgroup form."""
import functools
from collections import Counter

import numpy as np
import pytest

from edge264_amd import backend, packet as P, synth
from oracle.pyoracle import _dpb_array
from tests.test_dbk_emu import ALPHA, BETA, _load
from tests.test_hip_forms import decoders, options, run_batch

W, H, SPLIT_COL = 24, 9, 12
GOP = "IPP"
OFFSETS = (6, -6)
SEEDS = (31, 32)


def _place(mbx, mby, w, h):
    return "inter" if mbx < SPLIT_COL else "intra"


@functools.lru_cache(maxsize=None)
def packets(seed):
    g = synth.StreamSynth(W, H, seed, num_refs=1, mv_range=0, p_skip=1.0, residual_prob=0.0, place=_place, filter_offsets=OFFSETS)
    return [bytes(p) for p in g.gop(GOP)]


def census(oracle, pkts):
    """per P picture: macroblocks with every bS 0, macroblocks with a bS 4, steps of the first luma group / the chroma group whose whole
    diagonal has every bS 0, and -- on the third vertical luma edge of the intra macroblocks, whose eight samples nothing has filtered
    before it -- the lines that filter, and those that pass alpha and fail beta"""
    nb = P.frame_bytes(W, H)
    dpb = [np.zeros(nb + 64, np.uint8) for _ in range(6)] + [None] * 26
    out = []
    for pkt in pkts:
        pk = P.Packet(pkt)
        d = int(pk.hdr["dst_slot"])
        rec = [None if b is None else b.copy() for b in dpb]
        oracle.decode_frame(pkt, rec, 1)  # reconstruction only
        oracle.decode_frame(pkt, dpb, 3)
        if not len(np.nonzero(pk.mbs["kind"] == P.MB_INTER)[0]):
            continue
        bs = oracle.frame_bs(pkt, W * H).reshape(H, W, 32)
        zero = ~bs.any(axis=2)
        strong = (bs == 4).any(axis=2)
        luma_diag = [t for t in range(W + 8) if all(0 <= t - g < W and zero[g, t - g] for g in range(8))]
        chroma_diag = [t for t in range(W + H) if all(0 <= t - g < W and zero[g, t - g] for g in range(H))]
        y = rec[d][:W * 16 * H * 16].reshape(H * 16, W * 16).astype(int)
        qp = pk.mbs["qp"][:, 0].reshape(H, W).astype(int)
        filt = alpha_not_beta = 0
        for mby in range(H):
            for mbx in range(SPLIT_COL, W):
                assert (bs[mby, mbx].reshape(2, 4, 4)[0, 2] == 3).all()
                alpha, beta = ALPHA[min(max(qp[mby, mbx] + OFFSETS[0], 0), 51)], BETA[min(max(qp[mby, mbx] + OFFSETS[1], 0), 51)]
                s = y[mby * 16:mby * 16 + 16, mbx * 16 + 6:mbx * 16 + 10]  # p1 p0 | q0 q1
                a = np.abs(s[:, 1] - s[:, 2]) < alpha
                b = (np.abs(s[:, 0] - s[:, 1]) < beta) & (np.abs(s[:, 3] - s[:, 2]) < beta)
                filt += int((a & b).sum())
                alpha_not_beta += int((a & ~b).sum())
        out.append(dict(zero=zero, strong=strong, luma_diag=luma_diag, chroma_diag=chroma_diag, filt=filt, alpha_not_beta=alpha_not_beta))
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_pictures_are_what_they_claim(oracle, seed):
    got = census(oracle, packets(seed))
    assert len(got) == GOP.count("P")
    left = np.arange(W)[None, :].repeat(H, 0) < SPLIT_COL
    for c in got:
        assert np.array_equal(c["zero"], left), "every bS 0 in the left half and nowhere else"
        assert np.array_equal(c["strong"], ~left), "a bS 4 record in every macroblock of the right half"
        assert c["luma_diag"] == list(range(7, SPLIT_COL)) and c["chroma_diag"] == list(range(H - 1, SPLIT_COL)), (c["luma_diag"], c["chroma_diag"])
        # (of 12 x 9 x 16 = 1728 lines; either kind on one line in seventeen means no step of the right half is without it)
        assert c["filt"] >= 100 and c["alpha_not_beta"] >= 100, (c["filt"], c["alpha_not_beta"])
    print(f"seed {seed}: per P picture {int(left.sum())} macroblocks with every bS 0, {int((~left).sum())} with a bS 4; third vertical edge of the intra macroblocks: "
          f"{[c['filt'] for c in got]} lines filter, {[c['alpha_not_beta'] for c in got]} pass alpha and fail beta")


@pytest.mark.parametrize("split", [0, 1], ids=["mixed_waves", "luma_and_chroma_waves"])
def test_kernel_source_on_the_host_agrees(oracle, split):
    """(CPU) the oracle and the kernel's source (tests/emu) agree on these packets"""
    emu = _load("libe264_pred_emu.so")
    nb = P.frame_bytes(W, H)
    dpb = [np.zeros(nb + 16, np.uint8) for _ in range(6)] + [None] * 26
    for i, pkt in enumerate(packets(SEEDS[0])):
        d = int(P.Packet(pkt).hdr["dst_slot"])
        mine = [None if b is None else b.copy() for b in dpb]
        oracle.decode_frame(pkt, mine, 1)
        prm = np.zeros(W * H * 146 + 64, np.uint8)
        assert emu.e264emu_dbkparam_frame(pkt, prm.ctypes.data) == 0
        assert emu.e264emu_deblock_frame2(pkt, _dpb_array(mine), prm.ctypes.data, split) == 0
        oracle.decode_frame(pkt, dpb, 3)
        bad = np.nonzero(mine[d] != dpb[d])[0]
        assert not len(bad), f"picture {i}: {len(bad)} bytes differ, first at {bad[:6].tolist()}"


@pytest.fixture(scope="module")
def device():
    dev = backend.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form,opts", [("dbk2_8", dict(split_planes=0)), ("dbk_planes", dict())], ids=["one_workgroup", "two_workgroups"])
def test_both_sides_of_every_join(device, oracle, form, opts):
    """waves 108: e264_deblock2_kernel<8> (one workgroup per picture) and e264_deblock2_planes_kernel<8> (luma and chroma on two)"""
    streams = [packets(s) for s in SEEDS]
    total = Counter()
    with options(device, waves=108, **opts) as cfg, decoders(device, len(streams)) as decs:
        for i in range(len(GOP)):
            total.update(run_batch(device, oracle, "resident", decs, [s[i] for s in streams], cfg, label=f"joins {form} picture {i} ({GOP[i]})"))
    assert total[form] == len(streams) * len(GOP) and not [f for f in total if f.startswith("dbk") and not f.startswith("dbkp") and f != form], total
