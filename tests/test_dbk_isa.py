"""What the deblocking walks pay at an edge's join, read from the compiled kernels (tools/isa_mix.py).

dk_edge (e264_dbk.h) ends in a join of up to three paths: no lane filters the edge, the bS < 4 filter, the bS 4 filter.  What meets there
must be the (up to six) results of the edge and nothing else: when the array of a line pair's twenty sample registers is carried across the
join instead, the compiler either splits every <2 x i16> register into halves and glues them together again (a v_lshrrev_b32 + v_perm_b32
pair that computes the identity, 13 - 18 of them per join in the chroma walk until round 7) or copies the array.  Both are properties of the
assembly, whatever the instruction counts of a given compiler: they are checked, the counts are not."""
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# edge joins of e264_deblock2_kernel: two walks (luma, chroma) x four unrolled steps x two phases (V, H) x four edge slots
JOINS = 2 * 4 * 2 * 4


@pytest.fixture(scope="module")
def mix():
    if not shutil.which(HIPCC):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mix.py"), "--json", "--kernel", "e264_deblock2"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_every_deblock2_kernel_is_there(mix):
    assert sorted(mix) == ["e264_deblock2_kernel<6>", "e264_deblock2_kernel<7>", "e264_deblock2_kernel<8>", "e264_deblock2_planes_kernel<8>"], sorted(mix)
    for name, k in mix.items():
        assert len(k["loops"]) == 2 and all(c["valu"] > 500 for c in k["loops"].values()), (name, k["loops"])  # the luma walk and the chroma walk


def test_no_identity_repack_pairs(mix):
    for name, k in mix.items():
        assert k["identity_pairs"] == 0, f"{name}: {k['identity_pairs']} v_lshrrev_b32 + v_perm_b32 pairs that compute the identity"


def test_no_array_copy_at_a_join(mix):
    """a copy of the line pair's array at every join is 20+ registers x 64 joins; the kernel as a whole (fetch-group hand-over, parameter
    sets, the early-out paths' two results included) moves fewer than four registers per join"""
    for name, k in mix.items():
        assert k["reg_moves"] < JOINS * 4, f"{name}: {k['reg_moves']} registers moved by v_mov_b32 / v_mov_b64, {JOINS} joins"
