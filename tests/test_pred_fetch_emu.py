"""The prediction kernel's one-trip phases on the HOST (tests/emu: the kernel's own body) against the oracle, on the 17 x 5 pictures of
tests/pred_fetch_cases.py: every shape of motion record in every quadrant beside every other, quadrants one list does not predict, the records that END the
motion section, and the macroblocks whose payload is the packet's last bytes or its first -- chroma DC alone, one 4x4 and one 8x8 luma block in byte form,
chroma AC without chroma DC, I_PCM.  The same packets then go, in heap blocks of exactly their size, through tests/emu/pred_fetch_asan (a stand-alone program
built with the address and undefined-behaviour sanitizers): a request that leaves the motion section or the macroblock's payload where that ends the packet
is reported there."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from edge264_amd import backend, packet as P
from oracle.pyoracle import Oracle, _dpb_array
from tests import pred_fetch_cases as F
from tests.test_pred_emu import mb_mask

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU], check=True, stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(EMU, "libe264_pred_emu.so"))
    lib.e264emu_pred_frame.argtypes = [C.c_char_p, C.c_void_p]
    lib.e264emu_pred_frame.restype = C.c_int
    return lib


def test_the_cases_are_what_they_say():
    """each payload picture holds the macroblock its name says, where it says, owning the bytes it says; "last" ends the packet, "first" starts the payload"""
    n = F.W * F.H
    seen = set()
    for name, ft, pkt in F.payload_pictures():
        assert backend.packet_check(pkt) == 0, (name, ft)
        if ft == "I":
            continue
        case, placement = name.split("@")
        seen.add((case, placement, ft))
        pk = P.Packet(pkt)
        assert (pk.width_mbs, pk.height_mbs) == (F.W, F.H) and len(pkt) == int(pk.hdr["total_bytes"])
        addr = F.special_addr(placement)
        m = pk.mbs[addr]
        owners = [a for a in range(n) if F.mb_payload_bytes(pk.mbs[a])]
        assert owners == [0, n - 1], (name, ft, owners)  # the case's macroblock and the ordinary one
        own = F.mb_payload_bytes(m)
        assert own == F.PAYLOADS[case][1], (name, ft, own)
        coded, flags = int(m["coded"]), int(m["flags"])
        if case == "chroma_dc_only":
            assert m["kind"] == P.MB_INTER and coded == P.CODED_CHROMA_DC
        elif case == "luma4x4_bytes":
            assert m["kind"] == P.MB_INTER and bin(coded).count("1") == 1 and coded & 0xffff and flags & P.MBF_LEV8 and not flags & P.MBF_T8x8
        elif case == "luma8x8_bytes":
            assert m["kind"] == P.MB_INTER and bin(coded).count("1") == 1 and coded & 0x1111 and flags & P.MBF_LEV8 and flags & P.MBF_T8x8
        elif case == "chroma_ac_no_dc":
            assert m["kind"] == P.MB_INTER and coded >> 16 & 0xff and not coded & P.CODED_CHROMA_DC and not coded & 0xffff
        else:
            assert m["kind"] == P.MB_PCM
        other = pk.mbs[n - 1 - addr]
        assert other["kind"] == P.MB_INTER and int(other["coded"]) == 1 and not int(other["flags"]) & P.MBF_LEV8
        if placement == "last":  # payload_off + payload = total_bytes
            assert int(pk.hdr["payload_off"]) + int(m["payload_off"]) + own == int(pk.hdr["total_bytes"]) == len(pkt), (name, ft)
            assert int(other["payload_off"]) == 0
        else:
            assert int(m["payload_off"]) == 0 and int(other["payload_off"]) >= own, (name, ft)
    assert seen == {(c, p, ft) for c in F.PAYLOADS for p in F.PLACEMENTS for ft in "PB"}
    # the motion pictures: tests/test_motion_fetch_emu.py::test_the_cases_are_what_they_say holds them to their names; here, that they are the size meant
    assert all((P.Packet(p).width_mbs, P.Packet(p).height_mbs) == (F.W, F.H) for _, _, p in F.motion_pictures())
    und = [P.Packet(p) for _, ft, p in F.motion_pictures(decodable=False) if ft == "B"]
    assert und and all((pk.motion["refPic"][pk.mbs["kind"] == P.MB_INTER].reshape(-1, 2, 4).max(1) < 0).any() for pk in und)  # quadrants no list predicts


def test_pred_fetch_emu(emu):
    """every stream's I, P, B pictures: what the kernel's body leaves in the samples it owns equals the oracle's reconstruction"""
    orc = Oracle()
    w, h = F.W, F.H
    nb = P.frame_bytes(w, h)
    sY = w * 16
    for name, pkts in F.streams().items():
        rng = np.random.default_rng(len(name))
        dpb = [rng.integers(0, 256, nb + 16, dtype=np.uint8) for _ in range(P.MAX_SLOTS)]
        for ft, pkt in zip("IPB", pkts):
            d = int(P.Packet(pkt).hdr["dst_slot"])
            mine = [b.copy() for b in dpb]
            before = mine[d].copy()
            orc.decode_frame(pkt, dpb, 1)  # reconstruction only
            assert emu.e264emu_pred_frame(pkt, _dpb_array(mine)) == 0
            my, mc = mb_mask(pkt, w, h)
            mask = np.concatenate([my.reshape(-1), np.concatenate([mc, mc], axis=1).reshape(-1)])
            bad = (mine[d][:nb] != dpb[d][:nb]) & mask
            assert not bad.any(), f"{name} {ft}: differs at bytes {np.nonzero(bad)[0][:6].tolist()} (luma rows are {sY} bytes, chroma starts at {sY * h * 16})"
            assert np.array_equal(mine[d][:nb][~mask], before[:nb][~mask]), f"{name} {ft}: samples the kernel does not own were written"


def test_pred_fetch_stays_inside_the_packet(tmp_path):
    """every picture, in a heap block of exactly its size, through the kernel's body under the sanitizers (a child process)"""
    exe = str(tmp_path / "pred_fetch_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "pred_fetch_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    path = tmp_path / "packets.bin"
    count = 0
    with open(path, "wb") as f:
        for pics in (F.motion_pictures(), F.motion_pictures(decodable=False), F.payload_pictures()):
            for name, ft, pkt in pics:
                f.write(struct.pack("<II", len(pkt), 1 if ft == "I" else 0))
                f.write(pkt)
                count += 1
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count(": 0, ") == count, r.stdout[-2000:]
