"""The parameter kernel's trips to memory, read from the compiled kernel (tools/isa_mix.py).

e264_dbkparam2_kernel is phases of loads between workgroup barriers, and its time is the latency of a workgroup divided by the eight that a CU holds:
every wait that has a load behind it is a round trip on that chain.  The data need two trips -- the records, then the motion they point at.  So in
the load segment and in the expansion segment of both forms no global load may execute after a memory wait of that segment (until round 8 the
quadrants' conditional loads made up to eight serial trips per list, with 11 / 23 waits between 14 / 21 loads), and what meets at the expansion's
joins must not be the 16-dword vector array (112 of that segment's 164 VALU instructions were v_mov).  Both are properties of the assembly, whatever
the instruction counts of a given compiler: they are checked, the counts are not.

What counts as "behind a wait" (tools/isa_mix.py): a global load that can execute after a memory wait of its segment WHICH HAD A GLOBAL LOAD OF THAT SEGMENT
TO WAIT FOR.  The kernel's prologue is part of the load segment: open_frame reads the destination slot's pointer with a flat load and waits for it before
any record is asked for.  That flat load is not counted as a load and its wait is not counted as the segment's first wait -- it is one more (uniform)
trip, named in DESIGN.md section 4.2, but not one of the phase's own; counted literally, "loads after the segment's first memory wait" would be EVERY load
of the load segment, in the parent tree as in this one."""
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORMS = ["e264_dbkparam2_kernel<false>", "e264_dbkparam2_kernel<true>"]
LOAD, EXPAND = 0, 1  # segments: up to the first barrier, between the first and the second


@pytest.fixture(scope="module")
def mix():
    if not shutil.which(HIPCC):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mix.py"), "--json", "--kernel", "e264_dbkparam2"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_both_forms_are_there(mix):
    assert sorted(mix) == FORMS, sorted(mix)
    for name in FORMS:
        seg = mix[name]["segments"]
        assert len(seg) == 5, (name, len(seg))  # load | expansion | comparisons | pieces | store
        assert seg[LOAD]["loads"] >= 3 and seg[EXPAND]["loads"] >= 3, (name, seg)  # (the segments are the ones meant)
        assert all(s["loads"] == 0 for s in seg[2:]), (name, seg)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("segment", [LOAD, EXPAND], ids=["load", "expansion"])
def test_one_trip_per_segment(mix, form, segment):
    s = mix[form]["segments"][segment]
    print(form, segment, s)
    assert s["loads_after_wait"] == 0, f"{form} segment {segment}: {s['loads_after_wait']} of {s['loads']} global loads behind a memory wait ({s['vm_waits']} waits)"


@pytest.mark.parametrize("form", FORMS)
def test_no_vector_array_across_the_expansion_joins(mix, form):
    s = mix[form]["segments"][EXPAND]
    print(form, s)
    assert s["reg_moves"] < 32, f"{form}: {s['reg_moves']} registers moved by v_mov_b32 / v_mov_b64 in the expansion segment"
