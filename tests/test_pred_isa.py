"""The prediction kernel's trips to memory, read from the compiled kernel (tools/isa_mix.py --kernel e264_pred).

e264_pred_kernel is phases between workgroup barriers, and a tile passes through dependent trips to memory that other tiles have to fill: every wait that
has a load behind it is a round trip on that chain.  Since round 9 the phases that read the packet -- the records (setup), the motion and the I_PCM samples
(classify, once per list), the scaling lists, chroma DC words and levels (residual) -- make ONE trip each: requests, one wait, results.  So in those segments
no global load may execute after a memory wait of the segment.  The two item segments (the reference windows: one trip per item, a list longer than the
workgroup takes several) are not held to it.  These are properties of the assembly, whatever the instruction counts of a given compiler.

What counts as "behind a wait" is tools/isa_mix.py's convention, the one tests/test_dbkp_isa.py uses: a global load that can execute after a memory wait
of its segment WHICH HAD A GLOBAL LOAD OF THAT SEGMENT TO WAIT FOR.  The kernel's prologue is part of the setup segment: open_frame's scalar loads of the job
and the header and the destination slot's pointer are a uniform trip of their own in front of the phase, named in DESIGN.md section 4.2, not counted here.

Which segment is which is read from the loads alone: the kernel's barriers are not all on one path (the list-1 phases), so a segment is what runs from one
barrier of the text to a next one.  The two segments with the most loads are the item phases; of the others that load anything, the first is the setup, the
last ones the residual (its first pass, and the pass of a tile with more 4x4 blocks than threads), and the ones between are the classification of either list
(list 0's is reached a second time from the setup's barrier, through the single-wave form of the workgroup-wide OR that the compiler keeps)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNEL = "e264_pred_kernel"


@pytest.fixture(scope="module")
def segments():
    if not shutil.which(HIPCC):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_mix.py"), "--json", "--kernel", "e264_pred"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    mix = json.loads(out.stdout)
    assert list(mix) == [KERNEL], list(mix)
    return mix[KERNEL]["segments"]


def phases(seg):
    """{phase: indices of its segments}"""
    loading = [i for i, s in enumerate(seg) if s["loads"]]
    items = sorted(sorted(loading, key=lambda i: seg[i]["loads"])[-2:])
    rest = [i for i in loading if i not in items]
    return {"setup": rest[:1], "classify": [i for i in rest[1:] if i < items[1]], "items": items, "residual": [i for i in rest if i > items[1]]}


def test_the_segments_are_the_ones_meant(segments):
    ph = phases(segments)
    print(ph, [(s["loads"], s["vm_waits"], s["loads_after_wait"]) for s in segments])
    assert ph["setup"] == [0], ph
    assert len(ph["classify"]) >= 2 and len(ph["residual"]) >= 1, ph  # list 0's and list 1's; the residual's first pass
    assert ph["items"][0] > ph["classify"][0] and ph["classify"][-1] < ph["items"][1] < ph["residual"][0], ph  # setup, classify 0, items 0, classify 1, items 1, residual
    # the item segments are the ones that fetch windows: each asks for more than all the other phases together
    assert min(segments[i]["loads"] for i in ph["items"]) > sum(segments[i]["loads"] for k in ("setup", "classify", "residual") for i in ph[k]), ph
    assert segments[-1]["loads"] == 0  # the flush stores


@pytest.mark.parametrize("phase", ["setup", "classify", "residual"])
def test_one_trip_per_phase(segments, phase):
    for i in phases(segments)[phase]:
        s = segments[i]
        print(phase, i, s)
        assert s["loads_after_wait"] == 0, f"{phase}, segment {i}: {s['loads_after_wait']} of {s['loads']} global loads behind a memory wait ({s['vm_waits']} waits)"
