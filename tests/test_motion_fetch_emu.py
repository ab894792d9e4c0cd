"""The parameter kernel's one-trip motion fetch on the HOST (tests/emu: the kernel's own body, both forms) against the oracle, on the pictures of
tests/motion_fetch_cases.py: every shape of motion record in every quadrant beside every other, quadrants no list predicts, and the records that END the
motion section -- the longest one, a lone 8-byte one, a one-partition one -- as the picture's last macroblock, its first, and on either side of a workgroup
boundary.  The same packets then go, in heap blocks of exactly their size, through tests/emu/motion_fetch_asan (a stand-alone program built with the address
and undefined-behaviour sanitizers): a request that leaves the motion section where the section ends the packet is reported there."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from edge264_amd import packet as P
from oracle.pyoracle import Oracle
from tests import motion_fetch_cases as M
from tests.test_dbkp_emu import expected_ab

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # the compiler of tests/emu/Makefile


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU], check=True, stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(EMU, "libe264_pred_emu.so"))
    for f in (lib.e264emu_dbkparam_frame2, lib.e264emu_dbkparam_frame2_nol1):
        f.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
    lib.e264emu_dbk_pieces.argtypes = [C.c_void_p, C.c_void_p]
    lib.e264emu_dbk_pieces.restype = None
    return lib


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def test_the_cases_are_what_they_say():
    """the 17 x 5 pictures: every ordered pair of shapes side by side and one above the other in every quadrant; the end-of-section records end their packets"""
    pics = {(n, ft): P.Packet(p) for n, ft, p in M.pictures(17, 5)}
    pk = pics["shapes", "P"]
    dirs = np.ascontiguousarray(pk.mbs["modes"]).view("<u4").reshape(-1, 2)
    sub = lambda a, q: int(dirs[a, 1]) >> (10 + 2 * q) & 3
    for q in range(4):
        assert {(sub(a, q), sub(a - 1, q)) for a in range(85) if a % 17} == {(s, t) for s in range(4) for t in range(4)}
        assert {(sub(a, q), sub(a - 17, q)) for a in range(17, 85)} == {(s, t) for s in range(4) for t in range(4)}
    for (name, ft), pk in pics.items():
        if ft == "I" or name in ("shapes", "unused"):
            continue
        addr = M.placements(17, 5)[name.split("@")[1]]
        off, h = (int(x) for x in dirs_of(pk)[addr])
        size = M.record_bytes(h)
        assert int(pk.hdr["motion_off"]) + off + size == int(pk.hdr["payload_off"]), (name, ft)  # the record ends the section
        if name.startswith("longest"):
            assert size == (160 if ft == "B" else 80) and int(pk.hdr["payload_off"]) == int(pk.hdr["total_bytes"]) == len(pk.data), (name, ft)  # ... and the packet
        if name.startswith("only_inter"):
            assert size == 8 and int(pk.hdr["payload_off"]) - int(pk.hdr["motion_off"]) == 8 and int(pk.hdr["n_inter_mbs"]) == 1, (name, ft)
        if name.startswith("one_partition"):
            assert size == 8 and int(pk.hdr["payload_off"]) == int(pk.hdr["total_bytes"]), (name, ft)
    un = pics["unused", "B"]
    h = dirs_of(un)[:, 1]
    both = {(int(x) >> q & 1, int(x) >> (4 + q) & 1) for x in h for q in range(4)}
    assert both == {(0, 0), (0, 1), (1, 0), (1, 1)} and int(h[0]) & 0x3ff == 0  # (macroblock 0: an inter macroblock without a record)


def dirs_of(pk):
    return np.ascontiguousarray(pk.mbs["modes"]).view("<u4").reshape(-1, 2)


@pytest.mark.parametrize("w,h", M.SIZES, ids=[f"{w}x{h}" for w, h in M.SIZES])
def test_motion_fetch_emu(emu, orc, w, h):
    n = w * h
    for name, ft, pkt in M.pictures(w, h):
        pk = P.Packet(pkt)
        bs = orc.frame_bs(pkt, n).reshape(n, 32)
        ab = expected_ab(pk, w)
        for form, fn in (("<true>", emu.e264emu_dbkparam_frame2), ("<false>", emu.e264emu_dbkparam_frame2_nol1)):
            if form == "<false>" and ft == "B":  # (the launcher's choice for pictures without list-1 motion only)
                continue
            pieces = np.full((n, 144), 0x5A, np.uint8)
            raw = np.zeros((n, 64), np.uint8)
            assert fn(pkt, pieces.ctypes.data, raw.ctypes.data) == 0
            assert np.array_equal(raw[:, :32], bs), f"{name} {ft} {form}: bS differs at macroblocks {np.nonzero((raw[:, :32] != bs).any(1))[0][:8].tolist()}"
            assert np.array_equal(raw[:, 32:], ab), f"{name} {ft} {form}: alpha / beta / indexA differ"
            exp = np.zeros((n, 144), np.uint8)
            for a in range(n):
                emu.e264emu_dbk_pieces(raw[a].ctypes.data, exp[a].ctypes.data)
            assert np.array_equal(pieces, exp), f"{name} {ft} {form}: pieces differ"


def test_motion_fetch_stays_inside_the_packet(tmp_path):
    """every picture of every size, in a heap block of exactly its size, through the kernel's body under the sanitizers (a child process)"""
    exe = str(tmp_path / "motion_fetch_asan")
    r = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + EMU, "-w",
                        os.path.join(EMU, "motion_fetch_asan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    path = tmp_path / "packets.bin"
    count = 0
    with open(path, "wb") as f:
        for w, h in M.SIZES:
            for name, ft, pkt in M.pictures(w, h):
                f.write(struct.pack("<II", len(pkt), 1 if ft == "B" else 3))
                f.write(pkt)
                count += 1 if ft == "B" else 2
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count(": 0, ") == count, r.stdout[-2000:]
