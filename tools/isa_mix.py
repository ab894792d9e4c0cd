#!/usr/bin/env python3
"""Static instruction mix of the gfx950 kernels, read from the compiler's assembly (host only: hipcc cross-compiles, no GPU).

    isa_mix.py [-D NAME[=VALUE] ...] [--kernel FRAGMENT] [--json] [--asm FILE]

Per kernel: static VALU / SALU / LDS / vector-memory instruction counts, the twenty most frequent opcodes, s_nop, v_mov_b32 + v_mov_b64
(all of them, and the register-to-register ones counted in registers moved: a v_mov_b64 moves two), and the number of IDENTITY RE-PACK PAIRS:

    v_lshrrev_b32 t, 16, x
    ...                                   (same basic block, neither register written in between)
    v_perm_b32    x, t, x, sel            sel = 0x05040100: bytes 0, 1 of x and bytes 0, 1 of its own upper half  ->  x = x

which is what a <2 x i16> value costs when the compiler carries it across a join as two halves.  For the kernels whose
name contains "deblock" the loops at depth 2 are listed too: they are the walks of dk_walk_group (e264_kernels.hip), DK_GS unrolled steps each;
in e264_deblock2* the larger one is the luma walk.

For the kernels whose name contains "dbkparam" the SEGMENTS between the workgroup barriers are listed (key "segments"): a kernel made of phases of loads between
barriers takes as long as its dependent trips to memory, and a trip is a wait with a load behind it.  Per segment, along the control flow (not the order of the
text: the compiler lays blocks out as it likes): global loads, `s_waitcnt vmcnt(..)`, and loads_after_wait = the global loads that can execute after a memory
wait of the same segment that had a global load of the segment to wait for (a loop that holds a load and a wait counts, by its back edge); VALU and the
registers moved by v_mov_b32 / v_mov_b64.  Only global_load_* count as loads, and a wait counts only from the segment's first global load on: flat loads, and
waits that come before any global load of the segment, are left out -- in segment 0 that is the prologue's flat load of the destination slot's pointer
(open_frame) and its wait, a uniform trip of its own in front of the phase ("vm_waits" does include that wait).  Segment 0 is the load phase (with the kernel's prologue), segment 1 the expansion of the motion.

For the kernels whose name contains "e264_pred" the segments are listed with the same fields, cut differently: that kernel's barriers are not all on one path (its
list-1 phases are behind a branch), so segment 0 is what runs from the entry to a first barrier and segment k what runs from the k-th s_barrier of the text to a
next one; what two barriers lead to is counted in both (tests/test_pred_isa.py tells the phases apart by their loads; profiles/r09_isa_mix.txt names them).

--asm FILE analyses an assembly file that exists already (another tree's, for a side-by-side) instead of compiling this tree.
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "edge264_amd", "csrc", "e264_kernels.hip")
IDENTITY_SEL = 0x05040100
VMEM = ("global_", "buffer_", "flat_", "scratch_")
SALU_NOT = ("s_nop", "s_waitcnt", "s_endpgm", "s_barrier", "s_load_", "s_buffer_load_", "s_sleep", "s_setprio", "s_code_end")


def compile_asm(defs):
    """the flags of tests/test_kernel_resources.py, to assembly"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", SRC, "-o", out, "-w"] + ["-D" + d for d in defs]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode:
            sys.exit("hipcc failed:\n" + r.stderr[-3000:])
        with open(out) as f:
            return f.read()


def demangle(name):
    m = re.match(r"_Z\d+([A-Za-z0-9_]+?)(?:ILi(\d+)E|ILb(\d)E)?(?:Ev)?PK", name)
    if not m:
        return name
    return m.group(1) + (f"<{m.group(2)}>" if m.group(2) else f"<{'true' if m.group(3) == '1' else 'false'}>" if m.group(3) else "")


def regs(tok):
    """the 32-bit registers an operand names: v5 -> {v5}, v[4:5] -> {v4, v5}"""
    m = re.fullmatch(r"([vsa])(\d+)", tok)
    if m:
        return {tok}
    m = re.fullmatch(r"([vsa])\[(\d+):(\d+)\]", tok)
    if m:
        return {f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    return set()


def new_counts():
    return {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "smem": 0, "s_nop": 0, "v_mov": 0, "reg_moves": 0, "identity_pairs": 0, "instructions": 0}


def analyse(asm):
    """{kernel: counts + opcodes + walk loops}"""
    kernels = {}
    cur = None
    for line in asm.splitlines():
        m = re.match(r"(_Z\w+|[A-Za-z_]\w*):\s+; @", line)
        if m:
            cur = {"name": demangle(m.group(1)), "mangled": m.group(1), **new_counts(), "opcodes": collections.Counter(), "loops": collections.OrderedDict()}
            sel_regs, pending, loop, blk_label = set(), {}, None, None
            body = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            if "dbkparam" in cur["name"]:
                cur["segments"] = segments(body)
            elif "e264_pred" in cur["name"]:
                cur["segments"] = segments(body, by_barrier=True)
            kernels[cur["mangled"]] = cur
            cur = None
            continue
        body.append(line)
        code, _, comment = line.partition(";")
        code = code.strip()
        if re.match(r"\.LBB\d+_\d+:", code) or comment.lstrip().startswith("%bb."):  # a new basic block
            pending = {}
            label = code[2:-1] if code else None
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", comment)
            loop = m.group(1) if m and m.group(2) == "2" else None
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", comment)
            if m and m.group(1) == "2":
                loop = label
            blk_label = label
            continue
        m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", comment)
        if m and not code:  # (the second line of a loop header's label)
            loop = blk_label if m.group(1) == "2" else None
            continue
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        parts = code.split(None, 1)
        op = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", parts[0])
        ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        ops = [o.split()[0] for o in ops if o]
        tallies = [cur] + ([cur["loops"].setdefault(loop, new_counts())] if loop else [])
        kind = "valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else "vmem" if op.startswith(VMEM) else \
            "smem" if op.startswith(("s_load_", "s_buffer_load_")) else "salu" if op.startswith("s_") and not op.startswith(SALU_NOT) else None
        for c in tallies:
            c["instructions"] += 1
            if kind:
                c[kind] += 1
            if op == "s_nop":
                c["s_nop"] += 1
        cur["opcodes"][op] += 1
        dst = regs(ops[0]) if ops and (kind in ("valu", "salu", "lds", "vmem", "smem")) else set()
        if op == "s_mov_b32" and len(ops) == 2:
            try:
                val = int(ops[1], 0)
            except ValueError:
                val = None
            (sel_regs.add if val == IDENTITY_SEL else sel_regs.discard)(ops[0])
        elif dst & sel_regs:
            sel_regs -= dst
        if op in ("v_mov_b32", "v_mov_b64"):
            moved = len(regs(ops[1])) if len(ops) > 1 and ops[1].startswith("v") else 0
            for c in tallies:
                c["v_mov"] += 1
                c["reg_moves"] += moved
        if op == "v_perm_b32" and len(ops) == 4:
            is_sel = ops[3] in sel_regs or ops[3].lower() in ("0x5040100", "0x05040100")
            if is_sel and ops[0] == ops[2] and pending.get(ops[1]) == ops[0]:
                for c in tallies:
                    c["identity_pairs"] += 1
                del pending[ops[1]]
                continue
        for t in [t for t, x in pending.items() if t in dst or x in dst]:
            del pending[t]
        if op == "v_lshrrev_b32" and len(ops) == 3 and ops[1] == "16" and ops[2].startswith("v") and ops[0] != ops[2]:
            pending[ops[0]] = ops[2]
    for k in kernels.values():
        k["top_opcodes"] = k.pop("opcodes").most_common(20)
        k["loops"] = {h: c for h, c in k["loops"].items() if c["valu"] >= 64}  # (the walks; a wait loop has a handful of instructions)
    return kernels


def is_vm_wait(op, text):
    return op == "s_waitcnt" and ("vmcnt" in text or re.fullmatch(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)", text) is not None)


def segments(lines, by_barrier=False):
    """the inter-barrier segments of one kernel's assembly lines (see the module's text).  by_barrier: a kernel whose barriers are not all on one path
    (e264_pred_kernel: its list-1 phases): segment 0 is what runs from the entry to a first barrier, segment k what runs from the k-th s_barrier of the text
    to a next one; what two barriers lead to (the residual lists behind either list's items) is counted in both"""
    ins, labels = [], {}
    for line in lines:
        code = line.partition(";")[0].strip()
        m = re.match(r"(\.LBB\d+_\d+):", code)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        parts = code.split(None, 1)
        ins.append((re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", parts[0]), code, [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []))
    n = len(ins)

    def succ(i):
        op, _, ops = ins[i]
        out = []
        if op.startswith("s_cbranch") or op == "s_branch":
            if ops and ops[-1] in labels and labels[ops[-1]] < n:
                out.append(labels[ops[-1]])
        if op not in ("s_branch", "s_endpgm") and i + 1 < n:
            out.append(i + 1)
        return out

    seg = [None] * n  # barriers passed on the way to an instruction
    work = [0] if n else []
    if n:
        seg[0] = 0
    while work:
        i = work.pop()
        for j in succ(i):
            if seg[j] is None:
                seg[j] = seg[i] + (ins[i][0] == "s_barrier")
                work.append(j)

    def flood(starts):
        """instructions that can execute after one of `starts` without passing a barrier"""
        seen, work = set(), [i for i in starts if ins[i][0] != "s_barrier"]
        while work:
            i = work.pop()
            for j in succ(i):
                if j not in seen:
                    seen.add(j)
                    if ins[j][0] != "s_barrier":
                        work.append(j)
        return seen

    is_load = [op.startswith("global_load_") for op, _, _ in ins]
    after_load = flood([i for i in range(n) if is_load[i] and seg[i] is not None])
    waits = [i for i in range(n) if seg[i] is not None and is_vm_wait(ins[i][0], ins[i][1])]
    after_wait = flood([i for i in waits if i in after_load])
    out = []
    if by_barrier:
        bars = [i for i in range(n) if ins[i][0] == "s_barrier" and seg[i] is not None]
        members = [flood([0]) | {0}] + [flood(succ(b)) | set(succ(b)) for b in bars] if n else []
    else:
        members = [{i for i in range(n) if seg[i] == k} for k in range(max([x for x in seg if x is not None], default=-1) + 1)]
    for member in members:
        c = {"loads": 0, "vm_waits": 0, "loads_after_wait": 0, "valu": 0, "v_mov": 0, "reg_moves": 0}
        for i in sorted(member):
            op, text, ops = ins[i]
            c["loads"] += is_load[i]
            c["vm_waits"] += is_vm_wait(op, text)
            c["loads_after_wait"] += is_load[i] and i in after_wait
            c["valu"] += op.startswith("v_")
            if op in ("v_mov_b32", "v_mov_b64"):
                c["v_mov"] += 1
                c["reg_moves"] += len(regs(ops[1].split()[0])) if len(ops) > 1 and ops[1].startswith("v") else 0
        out.append(c)
    return out


def report(kernels, out=sys.stdout):
    for k in kernels.values():
        print(f"{k['name']}", file=out)
        print(f"   VALU {k['valu']}  SALU {k['salu']}  LDS {k['lds']}  VMEM {k['vmem']}  SMEM {k['smem']}  |  s_nop {k['s_nop']}  v_mov {k['v_mov']} "
              f"(registers moved {k['reg_moves']})  identity re-pack pairs {k['identity_pairs']}", file=out)
        if "deblock" in k["name"]:
            for h, c in k["loops"].items():
                print(f"   walk loop {h}: VALU {c['valu']}  LDS {c['lds']}  VMEM {c['vmem']}  s_nop {c['s_nop']}  v_mov {c['v_mov']} (registers moved {c['reg_moves']})  "
                      f"identity pairs {c['identity_pairs']}", file=out)
        for i, c in enumerate(k.get("segments", [])):
            print(f"   segment {i}: global loads {c['loads']}  s_waitcnt vmcnt {c['vm_waits']}  loads after a wait {c['loads_after_wait']}  |  VALU {c['valu']}  "
                  f"v_mov {c['v_mov']} (registers moved {c['reg_moves']})", file=out)
        print("   " + "  ".join(f"{op} {n}" for op, n in k["top_opcodes"]), file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-D", dest="defs", action="append", default=[], help="an extra preprocessor definition, as for hipcc")
    ap.add_argument("--kernel", help="only kernels whose name contains this")
    ap.add_argument("--json", action="store_true", help="one JSON object {kernel name: figures} instead of the table")
    ap.add_argument("--asm", help="analyse this assembly file instead of compiling")
    args = ap.parse_args()
    if args.asm:
        with open(args.asm) as f:
            asm = f.read()
    else:
        asm = compile_asm(args.defs)
    kernels = {m: k for m, k in analyse(asm).items() if not args.kernel or args.kernel in k["name"]}
    if args.json:
        json.dump({k["name"]: {n: v for n, v in k.items() if n not in ("name",)} for k in kernels.values()}, sys.stdout, indent=1)
        print()
    else:
        report(kernels)
    return 0


if __name__ == "__main__":
    sys.exit(main())
