#!/usr/bin/env python3
"""bench.py -- 1080p frames/s of the MI355X macroblock-reconstruction back end.

One "step" = one pass of the hot path over one batch of synthetic input: every stream of this rank decodes one GOP
(default IPPPPPPP, 1080p High profile, BASELINE.json configs[2]: 6-tap luma / bilinear chroma MC + 4x4 and 8x8 residual +
in-loop deblocking; frame 0 is an all-intra I frame).  Command packets and DPBs are resident in HBM before the timed region;
each stream has its OWN copy of the packets and its own DPB (no cross-stream cache sharing).

Streams are independent, so N GPUs = N x the same per-GPU work (weak scaling), no collective on the data path;
torch.distributed (RCCL) is used only for the barrier and the max-over-ranks of the elapsed time.  `--gpus N` without a
torchrun environment launches the N ranks itself (torch.distributed.run, one process per GPU).

Prints ONE JSON line (rank 0).  One submission (= one frame of every stream) is four kernel launches on the back end's
queue: e264_dbkparam2_kernel (bS / alpha / beta), e264_pred_kernel (inter prediction + residual, tile-parallel),
e264_intra_kernel (intra wavefront), e264_deblock_kernel (deblocking wavefront).  With --lanes L > 1 the streams are split
into L groups bound to L compute lanes (HIP queues) of the device: group g's submission of frame f runs beside the other
groups' (streams are independent), the tile-parallel kernels of one lane filling the compute units the wavefront kernels of
another leave idle.  Kernel times are measured live with HIP events recorded on the lanes around each launch (with several
lanes a launch's duration includes the time it shares the GPU with the other lanes' kernels).

roofline (all per submission of one frame of every stream of one GPU; DESIGN.md section 4 states the figures):
  kernels[k].own_bytes  the bytes kernel k has to move as the pass it is: the samples it writes, the samples it reads,
                        the command bytes it consumes (sample and command bytes kept apart);
  kernel / achieved / frac   the DOMINANT kernel (largest share of the submission) against ITS OWN bytes;
  end_to_end            SURVEY.md 8(d)'s algorithmic bytes of the submission (every sample written once, reference samples
                        read once per prediction direction, command bytes consumed -- the fused ideal, so the second pass of
                        the separate deblocking kernel counts as time but not as bytes) / the time of all four kernels;
  traffic               HBM-side bytes of the dominant kernel from the PMC passes committed under profiles/ (canned, matched
                        on the configuration), else null.
cpu_baseline: the unmodified reference decoder on the host cores (oracle/cpu_baseline.py), plus the reference's own SIMD
kernels replaying the bench packets on one core (`kernel_replay`).

A plain run does what the headline needs and no more: it builds the synthetic GOPs (one worker process per GOP, while this
process sets up the device), uploads them, warms up, times the steps, writes --dump-outputs and prints the line, roofline
included (its kernel times are taken live in the timed steps, its counters come from files).  `--full` adds the rest:
`verify` / `bit_exact` (every stream and frame of one more GOP against the CPU oracle), `cpu_baseline`, `other_configs`,
`staggered_gops`, `same_input`, `system`, `pcie_inclusive` and `single_stream`; in a plain line these keys are null.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
KERNELS = ["e264_dbkparam2_kernel", "e264_pred_kernel", "e264_intra_kernel", "e264_deblock_kernel"]
SIDE_QUEUE_DEFAULT = 0
DBK_BYTES = 144  # deblocking parameters per macroblock (edge264_amd/csrc/e264_kernels.h)
DUMP_BYTES = 64 * 10**6  # --dump-outputs: both arrays together, headers included
DUMP_SEED = 2024  # --dump-outputs: the sample positions of stream k come from default_rng((DUMP_SEED, k))
# what only --full runs: a plain run is the headline alone (set up, warm up, time the steps, --dump-outputs, the line)
FULL_ONLY = ("no_verify", "no_cpu_baseline", "no_other_configs", "no_host_packets", "no_system", "no_staggered", "no_single_stream", "no_same_input")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="ranks = GPUs of this node; spawns them when not already under torchrun")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--streams", type=int, default=int(os.environ.get("E264_STREAMS", 256)), help="concurrent streams per GPU")
    ap.add_argument("--total-streams", type=int, default=None, help="streams of the WHOLE job, sharded over the ranks (strong scaling) instead of --streams per GPU")
    ap.add_argument("--config5", action="store_true", help="BASELINE configs[4]: 256 concurrent 1080p streams over the node's GPUs (= --total-streams 256; 32 per GPU at --gpus 8)")
    ap.add_argument("--no-numa-bind", action="store_true", help="leave the rank's CPU affinity alone (default: the CPUs of the GPU's NUMA node)")
    ap.add_argument("--gop", default=os.environ.get("E264_GOP", "IPPPPPPP"))
    ap.add_argument("--width-mbs", type=int, default=120)
    ap.add_argument("--height-mbs", type=int, default=68)
    ap.add_argument("--waves", type=int, default=int(os.environ.get("E264_WAVES", 108)), help="deblocking kernel: 108 (default) = 8 waves taking luma groups (8 rows) and chroma groups (15 rows) from one list, e264_deblock2_kernel; 2 / 4 / 7 / 8 = that many mixed waves of 5 rows, e264_deblock_kernel")
    ap.add_argument("--intra-waves", type=int, default=int(os.environ.get("E264_INTRA_WAVES", 16)))
    ap.add_argument("--cpu-seconds", type=float, default=8.0, help="bounded CPU baseline sample (per leg)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short runs of BASELINE configs[1] and configs[3] (N=1)")
    ap.add_argument("--no-host-packets", action="store_true", help="skip the PCIe-inclusive run (N=1)")
    ap.add_argument("--variants", type=int, default=int(os.environ.get("E264_VARIANTS", 4)), help="distinct synthetic GOPs (seeds 1234, 1235, ...): stream k decodes GOP k mod V, "
                    "so that the timed pictures and the verification are not copies of one GOP")
    ap.add_argument("--no-system", action="store_true", help="skip the system leg (e264_multi: parser + emitters + GPU on the container's cores, N=1)")
    ap.add_argument("--no-staggered", action="store_true", help="skip the leg with the streams' GOPs out of phase (N=1)")
    ap.add_argument("--no-single-stream", action="store_true", help="skip the single-stream latency leg (N=1)")
    ap.add_argument("--no-same-input", action="store_true", help="skip the same-input leg (the 1080p bitstream fixtures on the GPU next to the CPU reference, N=1)")
    ap.add_argument("--lanes", type=int, default=int(os.environ.get("E264_LANES", 1)), help="compute lanes (HIP queues): the streams are split into this many "
                    "groups whose submissions overlap on the GPU")
    ap.add_argument("--capture", default=None, help="capture file (edge264_amd/replay.py): its first stream's packets replace the synthetic GOP, "
                    "so that the kernels are timed on real motion / partition statistics (tools/make_capture.py writes one from a .264)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write the pictures the last timed step left in "
                    "rank 0's streams to DIR/pictures.npy and DIR/positions.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true", help="after the headline, run everything else the line can carry: the oracle check of every stream "
                    "and frame, the CPU baseline, the other configurations and the PCIe-inclusive, staggered, same-input, system and single-stream legs "
                    "(the --no-* options leave parts out); without it those keys are null")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        for flag in FULL_ONLY:
            setattr(args, flag, True)
    return args


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` outside torchrun: one process per GPU through torch.distributed.run; rank 0's JSON line
    is this process's stdout."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1")).returncode


def kernel_own_bytes(models, n_streams):
    """Per kernel: (sample bytes, command bytes) of one submission, averaged over the GOP's frames."""
    out = {}
    for name in KERNELS:
        sb = cb = 0.0
        for m in models:
            F, n = m["F"], m["n_mbs"]
            if name == "e264_dbkparam2_kernel":  # reads record headers + motion, writes the parameter records
                c, s_ = 32 * n + m["cmd_motion"] + DBK_BYTES * n, 0
            elif name == "e264_pred_kernel":  # writes its macroblocks, reads each reference sample once per direction
                s_ = F * m["inter"] + F * m["dirs"]
                c = 32 * n + m["cmd_motion"] + m["cmd_payload_inter"]
            elif name == "e264_intra_kernel":  # writes its macroblocks (neighbour rows are cache hits)
                s_ = F * m["intra"]
                c = 32 * n + m["cmd_payload_intra"]
            else:  # deblocking as a pass of its own: the frame read and written once, parameters read
                s_ = 2 * F
                c = 4 * n + DBK_BYTES * n
            sb += s_
            cb += c
        out[name] = (sb / len(models) * n_streams, cb / len(models) * n_streams)
    return out


def newest_traffic(dom, streams, gop, W, H, lanes, live_ms):
    """HBM-side bytes per launch of the dominant kernel from the NEWEST profiles/r*_hbm_traffic.json taken on this configuration
    (PMC passes cannot run inside a timed bench: separate rocprofv3 --pmc runs, tools/visits/gpu_profile_r4.sh).  Returns (bytes or None,
    a description that names the file, the kernel times it was taken at when it records them, and says so when the live
    times have moved more than 10 % away from them)."""
    import glob
    import re
    best = None
    for path in glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")):
        m = re.match(r"r(\d+)([a-z]?)_", os.path.basename(path))
        try:
            with open(path) as f:
                tj = json.load(f)
        except (OSError, ValueError):
            continue
        cfg = tj.get("config", {})
        if (cfg.get("streams"), cfg.get("gop"), cfg.get("width_mbs"), cfg.get("height_mbs"), cfg.get("lanes", 1)) != (streams, gop, W, H, lanes):
            continue
        key = (int(m.group(1)) if m else -1, m.group(2) if m else "", os.path.getmtime(path))
        if best is None or key > best[0]:
            best = (key, path, tj)
    if best is not None and dom == "e264_deblock_kernel" and dom not in best[2].get("kernels", {}) and "e264_deblock2_kernel" in best[2].get("kernels", {}):
        dom = "e264_deblock2_kernel"  # (the same kernel slot of the submission, taken with luma / chroma waves)
    if best is None or dom not in best[2].get("kernels", {}):
        return None, None
    _, path, tj = best
    src = {"file": os.path.relpath(path, ROOT), "how": "PMC passes (TCC_EA0_RDREQ* / WRREQ*), canned: not measured by this run"}
    at = tj.get("kernel_ms_per_launch")
    if at:
        src["taken_at_kernel_ms"] = at
        drift = {k: round(live / at[k] - 1.0, 3) for k, live in zip(KERNELS, live_ms) if at.get(k)}
        src["live_vs_taken"] = drift
        src["stale"] = any(abs(v) > 0.10 for v in drift.values())
    else:
        src["stale"] = None  # the file does not say which build it was taken on
    return int(best[2]["kernels"][dom]["hbm_bytes_per_launch"]), src


VALU_RATE_G = 0.54   # G wave-instructions/s per SIMD of the packed / VOP3 / byte-permute instructions the kernels are made of (tools/calib/valu_rate, profiles/r05_valu_rate.txt: 0.50 - 0.57; plain VOP2 adds / ands / shifts: 0.9)
N_SIMDS = 1024       # 256 CUs x 4


def newest_sq_mix(streams, gop, W, H):
    """per-kernel SQ counters per launch from the NEWEST profiles/r*_sq_mix.json of this configuration (tools/pmc_summary.py --sq-json; counters
    cannot be collected inside a timed run)"""
    import glob
    import re
    best = None
    for path in glob.glob(os.path.join(ROOT, "profiles", "r*_sq_mix.json")):
        m = re.match(r"r(\d+)([a-z]?)_", os.path.basename(path))
        try:
            with open(path) as f:
                tj = json.load(f)
        except (OSError, ValueError):
            continue
        cfg = tj.get("config", {})
        if (cfg.get("streams"), cfg.get("gop"), cfg.get("width_mbs"), cfg.get("height_mbs")) != (streams, gop, W, H):
            continue
        key = (int(m.group(1)) if m else -1, m.group(2) if m else "", os.path.getmtime(path))
        if best is None or key > best[0]:
            best = (key, path, tj)
    return (None, None) if best is None else (os.path.relpath(best[1], ROOT), best[2])


def issue_roofline(kern, sq_path, sq, samples_per_launch):
    """The roof the kernels are under: none of them is bound by bytes.  Per kernel, from the SQ counters of the newest
    canned PMC pass: VALU wave-instructions per launch, the share of the chip's VALU issue slots they take at the LIVE kernel time when
    priced at the packed / VOP3 rate (an upper bound: VOP2 instructions issue 1.7 x faster), and lane-level VALU instructions per picture sample."""
    if sq is None:
        return None
    out = {"source": sq_path, "rate_G_wave_instr_per_s_per_simd": VALU_RATE_G, "simds": N_SIMDS,
           "how": "valu_issue_frac = SQ_INSTS_VALU per launch / (simds x live seconds per launch x rate); counters canned (separate rocprofv3 --pmc pass), time live",
           "kernels": {}}
    for name, k in kern.items():
        c = sq["kernels"].get(name) or (sq["kernels"].get("e264_deblock2_kernel") if name == "e264_deblock_kernel" else None)
        if not c or "SQ_INSTS_VALU" not in c or k["ms_per_launch"] <= 0:
            continue
        valu = c["SQ_INSTS_VALU"]
        at = (sq.get("kernel_ms_per_launch") or {}).get(name)
        out["kernels"][name] = {"valu_wave_instr_per_launch": int(valu), "salu_wave_instr_per_launch": int(c.get("SQ_INSTS_SALU", 0)),
                                "lds_wave_instr_per_launch": int(c.get("SQ_INSTS_LDS", 0)), "vmem_wave_instr_per_launch": int(c.get("SQ_INSTS_VMEM", 0)),
                                "valu_issue_frac": round(valu / (N_SIMDS * k["ms_per_launch"] * 1e-3 * VALU_RATE_G * 1e9), 3),
                                "lane_instr_per_sample": round(valu * 64 / samples_per_launch, 2),
                                "counters_taken_at_ms": at, "stale": (abs(k["ms_per_launch"] / at - 1.0) > 0.10) if at else None}
    return out


def link_rate_gbs():
    """H2D rate of this box's link from page-locked memory (one 256-MiB copy, best of 4): what pcie_inclusive is a fraction of"""
    try:
        import torch
        if not torch.cuda.is_available():
            return None
        n = 256 << 20
        h = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        d = torch.empty(n, dtype=torch.uint8, device="cuda")
        best = 0.0
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            d.copy_(h, non_blocking=True)
            b.record()
            torch.cuda.synchronize()
            best = max(best, n / (a.elapsed_time(b) * 1e-3) / 1e9)
        del h, d
        return round(best, 2)
    except Exception:  # noqa: BLE001 -- informational
        return None


def single_stream_leg(dev, backend, gop_packets, W, H, n_slots, frame_nb, fill_value):
    """ONE 1080p stream (VERDICT r5 item 7 of "missing": what an integrator asks first).  (a) resident: the bench GOP's packets in HBM, one picture per
    submission, the host waits for every picture; (b) the edge264.h API: nat1080_ipp30.264 through edge264_decode_NAL / edge264_get_frame of
    libedge264_hipfront.so (parser + emitters + H2D + 4 kernels + download to the host mirror), the second of two runs."""
    out = {}
    st = backend.Stream(dev, W, H)
    st.frame_bytes = frame_nb
    for i in range(n_slots):
        st.alloc(i)
        st.fill(i, fill_value)
    dp = [dev.upload_packet(p) for p in gop_packets]
    bs = [dev.make_batch([st], [q]) for q in dp]
    for b in bs:
        dev.submit_prepared(b, backend.RUN_ALL)
    dev.sync()
    per = []
    for _ in range(3):
        for b in bs:
            t0 = time.perf_counter()
            dev.submit_prepared(b, backend.RUN_ALL)
            dev.sync()
            per.append(time.perf_counter() - t0)
    n = len(bs)
    ms = [1e3 * float(np.mean(per[f::n])) for f in range(n)]
    out["resident"] = {"ms_per_picture": round(float(np.mean(ms)), 3), "ms_first_picture_of_gop": round(ms[0], 3), "ms_other_pictures": round(float(np.mean(ms[1:])), 3) if n > 1 else None,
                       "pictures_per_s": round(1e3 / float(np.mean(ms)), 1),
                       "what": "one stream, packets resident, one submission (4 launches) per picture, host synchronises after each: two of the four kernels run ONE workgroup per picture"}
    for b in bs:
        dev.free_batch(b)
    for q in dp:
        q.free()
    st.close()
    try:
        from edge264_amd import front
        path = os.path.join(ROOT, "tests", "golden", "streams", "nat1080_ipp30.264")
        data = open(path, "rb").read()
        front.decode_timed(data)
        r = front.decode_timed(data)
        out["api"] = {"file": os.path.basename(path), "pictures": r["pictures"], "ms_per_picture": round(1e3 * r["seconds"] / max(r["pictures"], 1), 3),
                      "pictures_per_s": round(r["pictures"] / r["seconds"], 1), "first_picture_ms": round(1e3 * r["first_picture_seconds"], 3) if r["first_picture_seconds"] else None,
                      "edge264_alloc_ms": round(1e3 * r["alloc_seconds"], 3),
                      "what": "edge264_alloc / edge264_decode_NAL / edge264_get_frame on the HIP sink, one decoder, one thread: parser + emitters + validation + H2D + 4 kernels + "
                              "download of every output frame to the host; second run of the file in this process"}
    except Exception as e:  # noqa: BLE001
        out["api"] = {"unavailable": f"{type(e).__name__}: {e}"}
    return out


def staggered_leg(dev, backend, streams, dpk, vpk, groups, n_slots, fill_value, nb, verify):
    """GOPs OUT OF PHASE (round 6).  The headline decodes picture f of every stream in submission f: all I pictures share one submission, in which the intra kernel
    (one workgroup per picture) keeps every CU busy.  Independent streams have their I pictures anywhere: here stream k runs k mod G pictures ahead, so every
    submission holds I and P pictures in the GOP's proportion (a stream that starts inside its GOP predicts from the filled slots: deterministic, verified against
    the oracle decoding the same order).  `lockstep`: the four kernels over the whole submission, the I pictures' 2.7-ms intra pass with 7/8 of the CUs idle;
    `value`: the launcher's default -- that pass starts on a second queue at the beginning of the submission, beside the parameter and prediction kernels of the
    other pictures (E264Fork.n_nopred, edge264_amd/csrc/e264_kernels.h)."""
    from edge264_amd import packet as P
    G, V, lanes = len(dpk[0]), len(vpk), len(groups)

    def phase(k):
        return (k // lanes) % G
    bs = [[dev.make_batch([streams[k] for k in idx], [dpk[k][(f + phase(k)) % G] for k in idx]) for idx in groups] for f in range(G)]

    def one_pass():
        for row in bs:
            for b in row:
                dev.submit_prepared(b, backend.RUN_ALL)

    def refill():
        for st in streams:
            for i in range(n_slots):
                st.fill(i, fill_value)
    res = {"streams": len(streams), "gop_phase_of_stream_k": "k mod %d" % G}
    for label, split in (("lockstep", 0), ("split", 1)):
        dev.set_option("split_intra", split)
        refill()
        one_pass()
        dev.sync()
        dev.kernel_timing(True)
        t0 = time.perf_counter()
        for _ in range(3):
            one_pass()
        dev.sync()
        dt = time.perf_counter() - t0
        k4, l4 = dev.kernel_time_ms()
        dev.kernel_timing(False)
        res[label] = {"value": round(3 * G * len(streams) / dt, 1), "unit": "frames/s", "ms_per_submission": round(1e3 * dt / (3 * G), 3),
                      "kernel_ms_per_launch": {n: round(t / max(l4, 1), 4) for n, t in zip(KERNELS, k4)}}
    res["value"] = res["split"]["value"]
    res["unit"] = "frames/s"
    res["note"] = ("kernel_ms_per_launch.e264_intra_kernel of `split` is the lane's wait for the I pictures' intra pass on the second queue after its own kernels, "
                   "not that pass's duration")
    if verify:
        from oracle.pyoracle import Oracle
        refill()
        probe = list(range(min(G, len(streams))))  # one stream of every phase
        dpbs = {k: [np.full(nb + 64, fill_value, np.uint8) for _ in range(n_slots)] + [None] * (32 - n_slots) for k in probe}
        orcs = {k: Oracle() for k in probe}
        bad = 0
        for f in range(G):
            for b in bs[f]:
                dev.submit_prepared(b, backend.RUN_ALL)
            dev.sync()
            for k in probe:
                pkt = vpk[k % V][(f + phase(k)) % G]
                orcs[k].decode_frame(pkt, dpbs[k], 3)
                d = int(P.Packet(pkt).hdr["dst_slot"])
                bad += 0 if np.array_equal(streams[k].download(d), dpbs[k][d][:nb]) else 1
        res["bit_exact"] = bad == 0
        res["frames_compared"] = G * len(probe)
    for row in bs:
        for b in row:
            dev.free_batch(b)
    refill()
    return res


def same_input_leg(dev, backend, n_streams, cpu):
    """SAME INPUT on both sides (the shape of the reference's own `edge264_test -b`, /root/reference/src/edge264_test.c:482-542):
    the two committed 1080p Annex-B fixtures -- the files oracle/cpu_baseline.py times the unmodified CPU decoder on -- are
    parsed HERE by the reference's front end + our emitters (edge264_amd/front.py, capture sink), and the resulting command
    packets are decoded on the GPU by `n_streams` decoders at once: resident in HBM, and from pageable host memory with the
    H2D copy inside the timed region.  Every picture of four of the streams is compared with the oracle's replay of the packets."""
    from edge264_amd import front, packet as P
    from oracle.pyoracle import Oracle  # checker only: the comparison below
    sdir = os.path.join(ROOT, "tests", "golden", "streams")
    from oracle.cpu_baseline import FIXTURES_1080P  # (the list only: the files the CPU baseline decodes)
    files = [n for n in FIXTURES_1080P if os.path.exists(os.path.join(sdir, n))]
    res = {"files": files, "streams": n_streams, "per_file": {}}
    tot_frames = tot_res = tot_host = tot_pin = tot_parse = tot_pictures = tot_wire = tot_bytes = tot_wbytes = 0.0
    all_ok = True
    for name in files:
        with open(os.path.join(sdir, name), "rb") as f:
            data = f.read()
        packets, out_frames, parse_s = front.capture_packets(data)
        parsed = [P.Packet(p) for p in packets]
        h0 = parsed[0].hdr
        W, H = int(h0["width_mbs"]), int(h0["height_mbs"])
        nb = int(h0["plane_size_Y"]) + int(h0["plane_size_C"])
        used = 0
        for pk in parsed:
            used |= 1 << int(pk.hdr["dst_slot"]) | int(pk.hdr["ref_slots"])
        slots = [i for i in range(32) if used >> i & 1]
        sts = []
        for _ in range(n_streams):
            st = backend.Stream(dev, W, H)
            st.frame_bytes = nb
            for i in slots:
                st.alloc(i)
                st.fill(i, 0)
            sts.append(st)
        dpk = [[dev.upload_packet(p) for p in packets] for _ in sts]
        bs = [dev.make_batch(sts, [dpk[k][f] for k in range(n_streams)]) for f in range(len(packets))]
        for b in bs:  # warm-up pass
            dev.submit_prepared(b, backend.RUN_ALL)
        dev.sync()
        dev.kernel_timing(True)
        t0 = time.perf_counter()
        for b in bs:
            dev.submit_prepared(b, backend.RUN_ALL)
        dev.sync()
        t_res = time.perf_counter() - t0
        k4, l4 = dev.kernel_time_ms()
        dev.kernel_timing(False)
        hbs = [dev.prepare_host_batch(sts, [packets[f]] * n_streams) for f in range(len(packets))]
        for hb in hbs + hbs[:4]:  # a whole pass and four more (untimed): every slot of the back end's batch ring has seen the largest batch -- its staging buffers have grown -- before the clock starts
            dev.submit_host_prepared(hb, backend.RUN_ALL)
        dev.sync()
        REP = 3  # passes over the file inside each host-packet clock (one pass of 30 submissions is 75 ms: too short to tell 3 % apart)
        t0 = time.perf_counter()
        for _ in range(REP):
            for hb in hbs:
                dev.submit_host_prepared(hb, backend.RUN_ALL)
        dev.sync()
        t_host = (time.perf_counter() - t0) / REP
        # the front end's own road: packets that already sit in page-locked memory, validated by their producer (here: backend.packet_check once),
        # gathered into the batch's staging buffer and copied in ONE transfer -- no per-macroblock walk inside the clock.  One buffer per stream and
        # picture, as 256 decoders leave them (3.6 GB per file; until round 6 one buffer per picture was read by every stream: sixteen threads gathering the
        # same lines 256 times read 82 - 111 k from box to box, profiles/r06_ablations.txt item 17)
        for p in packets:
            assert backend.packet_check(p) == 0
        spins = [[dev.pinned_copy(p) for p in packets] for _ in range(n_streams)]
        pins = [pp for row in spins for pp in row]
        pbs = [dev.prepare_pinned_batch(sts, [spins[k][f] for k in range(n_streams)], [len(packets[f])] * n_streams) for f in range(len(packets))]
        for pb in pbs + pbs[:4]:
            dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(REP):
            for pb in pbs:
                dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        t_pin = (time.perf_counter() - t0) / REP
        for pp in pins:
            dev.pinned_free(pp)
        # the same road with the front end folding its packets (e264front_set_compact(1): the WIRE form, include/edge264_compact.h -- P_Skip / plain
        # 16x16 macroblocks without residual in 12 bytes instead of 40, unfolded on the device by e264_expand_kernel in front of the four kernels)
        wire, _, wire_parse_s = front.capture_packets(data, compact=True)
        front.capture_packets(b"", compact=False)
        assert len(wire) == len(packets)
        for p in wire:
            assert backend.packet_check(p) == 0
        wspins = [[dev.pinned_copy(p) for p in wire] for _ in range(n_streams)]
        wpins = [pp for row in wspins for pp in row]
        wbs = [dev.prepare_pinned_batch(sts, [wspins[k][f] for k in range(n_streams)], [len(wire[f])] * n_streams) for f in range(len(wire))]
        for pb in wbs + wbs[:4]:  # (the ring slots' expansion buffers are made here)
            dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(REP):
            for pb in wbs:
                dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        t_wire = (time.perf_counter() - t0) / REP
        # verification (untimed): one more pass from cleared slots, four streams, every picture -- resident version-4 packets, then the wire packets
        orc = Oracle()
        dpb = [np.zeros(nb + 64, np.uint8) if used >> i & 1 else None for i in range(32)]
        probe = sorted({0, n_streams // 3, 2 * n_streams // 3, n_streams - 1})
        bad = 0
        want = []
        for p in packets:
            orc.decode_frame(p, dpb, 3)
            want.append(dpb[int(P.Packet(p).hdr["dst_slot"])][:nb].copy())
        for form in ("resident", "wire"):
            for st in sts:
                for i in slots:
                    st.fill(i, 0)
            for f in range(len(packets)):
                if form == "resident":
                    dev.submit_prepared(bs[f], backend.RUN_ALL)
                else:
                    dev.submit_pinned_prepared(wbs[f], backend.RUN_ALL)
                dev.sync()
                d = int(parsed[f].hdr["dst_slot"])
                for k in probe:
                    bad += 0 if np.array_equal(sts[k].download(d), want[f]) else 1
        del want
        for pp in wpins:
            dev.pinned_free(pp)
        all_ok &= bad == 0
        n = len(packets) * n_streams
        res["per_file"][name] = {"pictures": len(packets), "packet_MB_per_picture": round(float(np.mean([len(p) for p in packets])) / 1e6, 3),
                                 "gpu_resident_frames_per_s": round(n / t_res, 1), "gpu_pcie_inclusive_frames_per_s": round(n / t_host, 1),
                                 "gpu_pcie_inclusive_pinned_frames_per_s": round(n / t_pin, 1),
                                 "wire_MB_per_picture": round(float(np.mean([len(p) for p in wire])) / 1e6, 3),
                                 "gpu_pcie_inclusive_pinned_wire_frames_per_s": round(n / t_wire, 1),
                                 "host_parse_emit_wire_frames_per_s_one_core": round(len(packets) / wire_parse_s, 1),
                                 "host_parse_emit_frames_per_s_one_core": round(len(packets) / parse_s, 1),
                                 "kernel_ms_per_launch": {n: round(t / max(l4, 1), 4) for n, t in zip(KERNELS, k4)},
                                 "pictures_compared": 2 * len(packets) * len(probe), "mismatching": bad}
        tot_frames += n; tot_res += t_res; tot_host += t_host; tot_pin += t_pin; tot_parse += parse_s; tot_pictures += len(packets)
        tot_wire += t_wire; tot_bytes += sum(len(p) for p in packets); tot_wbytes += sum(len(p) for p in wire)
        for b in bs:
            dev.free_batch(b)
        for row in dpk:
            for q in row:
                q.free()
        for st in sts:
            st.close()
    res.update({"gpu_resident_frames_per_s": round(tot_frames / tot_res, 1), "gpu_pcie_inclusive_frames_per_s": round(tot_frames / tot_host, 1),
                "gpu_pcie_inclusive_pinned_frames_per_s": round(tot_frames / tot_pin, 1),
                "gpu_pcie_inclusive_pinned_wire_frames_per_s": round(tot_frames / tot_wire, 1), "wire_bytes_over_packet_bytes": round(tot_wbytes / tot_bytes, 3),
                "host_parse_emit_frames_per_s_one_core": round(tot_pictures / tot_parse, 1) if tot_parse else None, "bit_exact": bool(all_ok),
                "what": "both sides decode the SAME files (two of random syntax, two from the procedural-video encoder tests/golden/nat_encoder.py): GPU = their command packets (reference parser + emitters, parsed in this process) decoded by "
                        f"{n_streams} concurrent decoders, packets resident in HBM / pageable host packets with validation + H2D inside the timed region / page-locked packets vetted by their producer (the front end's own road) with the H2D inside, as version-4 packets and in the wire form (version 5, include/edge264_compact.h: the front end folds P_Skip / plain 16x16 macroblocks, e264_expand_kernel unfolds them on the device); "
                        "CPU = the unmodified reference decoder on these files (cpu_baseline, same run).  The parser itself is host work on both sides: "
                        "host_parse_emit is what ONE core delivers, the GPU figures are what the device sustains behind enough parsing cores"})
    if cpu and cpu.get("value"):
        res["cpu_reference_frames_per_s"] = cpu["value"]
        res["cpu_cores"] = cpu["cores"]
        res["gpu_resident_vs_cpu_all_cores"] = round(res["gpu_resident_frames_per_s"] / cpu["value"], 2)
        res["gpu_pcie_inclusive_vs_cpu_all_cores"] = round(res["gpu_pcie_inclusive_frames_per_s"] / cpu["value"], 2)
    return res


def system_leg(cpu, seconds=12.0):
    """SYSTEM level (the shape of the reference's own whole-decoder clock, /root/reference/src/edge264_test.c:482-542): Annex-B bytes in, decoded
    pictures in HBM out, with the reference's parser + our emitters on the host cores INSIDE the clock: edge264_amd/e264_multi, 128 decoders
    (32 x the four 1080p fixtures `cpu_baseline` decodes), threads = the container's cores - 1 (one is left to the submitter and the back
    end's threads), packets assembled in page-locked memory and submitted in place, no read-back.  Two runs: parser + emitters alone
    (packets dropped: what the host delivers) and end to end (the same with the GPU behind it)."""
    from oracle.cpu_baseline import FIXTURES_1080P, STREAMS, cpu_quota, physical_cores  # (host-side helpers only: which cores, which files)
    exe = os.path.join(ROOT, "edge264_amd", "e264_multi")
    front = os.path.join(ROOT, "edge264_amd", "libedge264_hipfront.so")
    hip = os.path.join(ROOT, "edge264_amd", "libedge264_hip.so")
    for f in (exe, front, hip):
        if not os.path.exists(f):
            return {"unavailable": f"{os.path.relpath(f, ROOT)} is not built"}
    quota = cpu_quota()
    cores = len(physical_cores()) if quota is None else max(1, min(len(physical_cores()), int(quota)))
    threads = max(1, cores - 1)
    names = [n for n in FIXTURES_1080P if os.path.exists(os.path.join(STREAMS, n))]
    files = [os.path.join(STREAMS, n) for n in names]
    repeat = max(1, 128 // len(names))
    res = {"streams": repeat * len(names), "threads": threads, "cores": cores, "files": names}
    for key, flag in (("parse_only", "--parse-only"), ("end_to_end", "--no-download")):
        loops = 2
        out = None
        for _ in range(3):  # a short run sizes the long one: ~`seconds` of wall clock each
            cmd = [exe, "--front", front, "--hip", hip, flag, "--threads", str(threads), "--repeat", str(repeat), "--stay", "--loops", str(loops)] + files
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
            if r.returncode != 0 or line is None:
                return {**res, "unavailable": f"e264_multi {flag}: rc {r.returncode}: {(r.stderr or r.stdout)[-300:]}"}
            out = json.loads(line)
            if out["seconds"] >= 0.6 * seconds:  # (long enough that the first loop's page-locking of ~400 packet buffers and first touches do not set the figure)
                break
            loops = max(loops + 1, int(loops * seconds / max(out["seconds"], 0.05)))
        st = out.get("steady") or {}
        steady = st.get("frames_per_s", 0) > 0
        res[key] = {"frames_per_s": st["frames_per_s"] if steady else out["frames_per_s"],
                    "decode_ms_per_picture": st["decode_ms_per_picture"] if steady else out.get("decode_ms_per_picture"),
                    "steady_state": steady, "after_seconds": st.get("after_seconds"),
                    "whole_run": {"frames_per_s": out["frames_per_s"], "frames": out["frames"], "seconds": out["seconds"], "loops": loops,
                                  "decode_ms_per_picture": out.get("decode_ms_per_picture")},
                    "frames": out["frames"], "avg_batch": out.get("avg_batch"), "thread_seconds": out.get("thread_seconds")}
    po, ee = res["parse_only"], res["end_to_end"]
    res["end_to_end_vs_parse_only"] = round(ee["frames_per_s"] / po["frames_per_s"], 3)
    if ee.get("decode_ms_per_picture"):
        res["host_cores_for_1000_streams_1080p30"] = round(30000.0 * ee["decode_ms_per_picture"] / 1e3, 1)
    if cpu and cpu.get("value"):
        res["cpu_reference_frames_per_s"] = cpu["value"]
        # the CPU baseline is a whole-run figure: divided into the WHOLE-RUN rate (start-up inside); the steady-state ratio beside it, named as such
        res["vs_cpu_reference_same_cores"] = round(ee["whole_run"]["frames_per_s"] / cpu["value"], 2)
        res["vs_cpu_reference_same_cores_steady_state"] = round(ee["frames_per_s"] / cpu["value"], 2)
    res["steady_state_note"] = ("frames_per_s / decode_ms_per_picture are STEADY-STATE figures: everything after the first loop's worth of pictures.  The first loop "
                                "allocates every decoder's device frames, page-locked mirrors and packet buffers inside the clock (~1.5 s for 128 decoders: "
                                "profiles/r05_host.txt item 4); `whole_run` includes it")
    res["what"] = ("whole decoder, host included: Annex-B bytes -> reference parser + emitters on `threads` host threads -> page-locked packets submitted in place "
                   "-> 4 kernels per batch -> pictures in HBM (no read-back); `parse_only` = the same host work with the packets dropped.  The device rates of "
                   "`value` / `same_input` need ~30000 x decode_ms_per_picture / 1000 parsing cores per GPU at 1000 x 1080p30")
    return res


def dump_outputs(out_dir, streams, parsed, frame_nb):
    """--dump-outputs: what a caller of the timed path receives from its last step, i.e. the decoded pictures still held in each
    stream's DPB (the last picture written into each slot the GOP writes, oldest first), as samples 0..255.
      pictures.npy   float32 [stream, picture, sample]
      positions.npy  float64 [stream, sample]: byte offsets of the samples into the picture (Y plane, then the chroma planes)
    When every sample of every picture does not fit into DUMP_BYTES, stream k keeps the same K positions in all its pictures,
    drawn without replacement by default_rng((DUMP_SEED, k)): the same arguments give the same positions in every run."""
    last = {int(q.hdr["dst_slot"]): f for f, q in enumerate(parsed)}
    slots = sorted(last, key=last.get)
    n, m = len(streams), len(slots)
    k = min(frame_nb, (DUMP_BYTES - 1024) // (n * (4 * m + 8)))  # 1024: the two .npy headers
    pictures = np.empty((n, m, k), np.float32)
    positions = np.empty((n, k), np.float64)
    for i, st in enumerate(streams):
        idx = np.arange(frame_nb) if k == frame_nb else np.sort(np.random.default_rng((DUMP_SEED, i)).choice(frame_nb, k, replace=False))
        positions[i] = idx
        for j, s in enumerate(slots):
            pictures[i, j] = st.download(s)[idx]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "pictures.npy"), pictures)
    np.save(os.path.join(out_dir, "positions.npy"), positions)


def synth_gop(W, H, seed, kw, gop):
    """One synthetic GOP and the traffic model of each of its packets.  Runs in a worker process: a 1080p GOP is seconds of pure Python,
    and the GOPs of the variants are independent of each other and of the device's set-up."""
    from edge264_amd import packet as P, synth
    packets = synth.StreamSynth(W, H, seed=seed, **kw).gop(gop)
    return packets, [P.Packet(p).traffic_model() for p in packets]


def main() -> int:
    args = parse_args()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus and args.gpus > 1:
        return launch_ranks(args.gpus)

    # stdout carries exactly ONE line (the JSON): libraries that chat on fd 1 (the RCCL version banner) go to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    from edge264_amd.sharding import bind_rank_to_gpu_socket, gather_rates, rank_info, reduce_elapsed, shard_streams
    rank, local_rank, world = rank_info()
    if args.config5:
        args.total_streams = 256
    if args.gpus is not None and args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a number for the wrong GPU count", file=sys.stderr)
        return 2
    # weak scaling (default): rank r owns streams shard_streams(streams * world, r, world) (= `streams` of them);
    # --total-streams / --config5: the job's streams are fixed and sharded (strong scaling)
    strong = args.total_streams is not None
    my_streams = len(shard_streams(args.total_streams if strong else args.streams * world, rank, world))
    if my_streams == 0:
        print(f"bench.py: rank {rank} of {world} has no stream to decode (--total-streams {args.total_streams})", file=sys.stderr)
        return 2

    from edge264_amd import packet as P, synth

    W, H = args.width_mbs, args.height_mbs
    ALL_I = (P.MB_I4x4, P.MB_I8x8, P.MB_I16x16)
    head_i = tuple(k for k, n in zip(ALL_I, ("4", "8", "16")) if n in os.environ.get("E264_I_KINDS", "4,8,16").split(","))  # measuring aid: intra kinds of the synthetic GOP
    fill_value = 128
    if args.capture:
        # ---- captured packets of a real bitstream (reference front end -> our emitters), first stream of the file ----
        from edge264_amd import replay
        cap = replay.Capture.load(args.capture)
        packets = cap.of_stream(cap.stream_ids()[0])
        parsed = [P.Packet(p) for p in packets]
        W, H = int(parsed[0].hdr["width_mbs"]), int(parsed[0].hdr["height_mbs"])
        args.gop = f"capture:{os.path.basename(args.capture)}:{len(packets)} pictures"
        fill_value = 0
        args.no_other_configs = True
    else:
        # ---- synthetic input (same bytes on every rank: seeded) -------------------------------
        skw = dict(t8x8=True, i_kinds=head_i, num_refs=2, residual_prob=float(os.environ.get("E264_RESIDUAL_PROB", 0.3)))
        skw.update(json.loads(os.environ.get("E264_SYNTH_KW", "{}")))  # measuring aid (tools/visits/gpu_sweep.sh): what each kernel's time depends on
        # one worker process per GOP, started before this process imports torch and opens the device, which it does meanwhile;
        # spawned, not forked: the workers start from a fresh interpreter and never touch the GPU
        import concurrent.futures
        import multiprocessing
        n_var = max(1, args.variants)
        pool = concurrent.futures.ProcessPoolExecutor(max_workers=min(n_var, len(os.sched_getaffinity(0))), mp_context=multiprocessing.get_context("spawn"))
        gop_jobs = [pool.submit(synth_gop, W, H, 1234 + v, skw, args.gop) for v in range(n_var)]
    # a run with any of the measuring aids set does not measure BASELINE configs[2] any more: the line says so (config.synth_overrides, workload)
    synth_overrides = {k: os.environ[k] for k in ("E264_I_KINDS", "E264_RESIDUAL_PROB", "E264_SYNTH_KW") if os.environ.get(k) and not args.capture}

    import importlib
    backend = importlib.import_module(os.environ.get("E264_BENCH_BACKEND", "edge264_amd.backend"))  # tests: a stub device on CPU ranks
    stub = getattr(backend, "IS_STUB", False)
    import torch
    dist = None
    tdev = torch.device("cpu") if stub else torch.device("cuda", local_rank)
    if world > 1 or os.environ.get("E264_FORCE_DIST"):  # E264_FORCE_DIST: exercise the RCCL path on one GPU
        import torch.distributed as dist
        if stub:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=tdev)

    # host side of this rank next to its GPU: before the back end creates its threads
    launcher_affinity = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None
    numa = {"numa_node": -1, "bound": False, "cpus": 0} if (stub or args.no_numa_bind) else bind_rank_to_gpu_socket(local_rank)

    class launcher_cpus:
        """The CPU legs (cpu_baseline, system) run on the cores the LAUNCHER granted, not on the GPU's NUMA node this rank bound itself to:
        'all cores' must mean the host's (on a two-socket box the baseline was taken on half the machine and the GPU / CPU ratio
        was inflated).  The binding comes back afterwards."""
        def __enter__(self):
            self.bound = os.sched_getaffinity(0) if launcher_affinity is not None else None
            if launcher_affinity is not None and self.bound != launcher_affinity:
                os.sched_setaffinity(0, launcher_affinity)
            return self

        def __exit__(self, *exc):
            if self.bound is not None and self.bound != launcher_affinity:
                os.sched_setaffinity(0, self.bound)
            return False

    dev = backend.Device(local_rank)
    dev.set_option("waves", args.waves)
    if args.intra_waves:
        dev.set_option("intra_waves", args.intra_waves)
    side_queue = int(os.environ.get("E264_SIDE_QUEUE", SIDE_QUEUE_DEFAULT))  # 0: one queue; 1: parameter kernel beside the prediction kernel; 2: beside the intra kernel
    dev.set_option("side_queue", side_queue)
    dev.set_option("upload_queue", int(os.environ.get("E264_UPLOAD_QUEUE", 1)))

    if args.capture:
        vpk = [packets]
        models = [pk.traffic_model() for pk in parsed]
    else:
        gops = [job.result() for job in gop_jobs]
        pool.shutdown()
        vpk = [pk for pk, _ in gops]
        models = [m for _, ms in gops for m in ms]
        packets = vpk[0]
        parsed = [P.Packet(p) for p in packets]
    V = len(vpk)
    vparsed = [[P.Packet(p) for p in pk] for pk in vpk]
    for vp in vparsed:  # the variants differ in content only: same slots, same geometry
        assert [int(q.hdr["dst_slot"]) for q in vp] == [int(q.hdr["dst_slot"]) for q in parsed]
    used = 0
    for pk in (q for vp in vparsed for q in vp):
        used |= 1 << int(pk.hdr["dst_slot"]) | int(pk.hdr["ref_slots"])
    n_slots = max(used.bit_length(), 3)
    frame_nb = int(parsed[0].hdr["plane_size_Y"]) + int(parsed[0].hdr["plane_size_C"])

    streams, dpk = [], []
    for s in range(my_streams):
        st = backend.Stream(dev, W, H)
        st.frame_bytes = frame_nb
        for i in range(n_slots):
            st.alloc(i)
            st.fill(i, fill_value)
        streams.append(st)
        dpk.append([dev.upload_packet(p) for p in vpk[s % V]])  # per-stream copy of the command bytes (stream s decodes GOP s mod V)
    # compute lanes: group g = streams g, g + L, g + 2L, ...; one batch per (frame, group)
    lanes = max(1, min(args.lanes, getattr(backend, "MAX_LANES", 1), my_streams))
    groups = [list(range(g, my_streams, lanes)) for g in range(lanes)]
    for g, idx in enumerate(groups):
        for k in idx:
            streams[k].bind_lane(g)

    def make_batches(dp):
        return [[dev.make_batch([streams[k] for k in idx], [dp[k][f] for k in idx]) for idx in groups] for f in range(len(dp[0]))]

    def submit_frame(bs, mode):
        for b in bs:
            dev.submit_prepared(b, mode)
    batches = make_batches(dpk)
    dev.sync()

    def step():
        for bs in batches:
            submit_frame(bs, backend.RUN_ALL)

    def barrier():
        dev.sync()
        if not stub and torch.cuda.is_available():
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    barrier()
    dev.kernel_timing(True)
    t0 = time.perf_counter()
    dev.event_record(0)
    for _ in range(args.steps):
        step()
    dev.event_record(1)
    dev.sync()
    if not stub and torch.cuda.is_available():
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    my_frames = my_streams * len(packets) * args.steps
    my_elapsed = elapsed
    if dist is not None:
        dist.barrier()
        elapsed, total_frames = reduce_elapsed(elapsed, my_frames, dist, tdev)
    else:
        total_frames = my_frames
    rates = gather_rates(my_elapsed, my_frames, dist, tdev)
    kernel_ms4, launches = dev.kernel_time_ms()
    dev.kernel_timing(False)
    ev_ms = dev.event_elapsed_ms(0, 1)
    frames_per_step = total_frames // args.steps
    value = total_frames / elapsed
    if rank == 0 and args.dump_outputs:  # before the verification below refills the slots
        dump_outputs(args.dump_outputs, streams, parsed, frame_nb)

    # ---- bit-exactness at full size (untimed): EVERY stream, EVERY frame of one more GOP against the CPU oracle ----
    verify, bit_exact = None, None
    expect = None  # [variant][frame]: the oracle's picture (kept for the wire-form check of the PCIe-inclusive leg)
    if rank == 0 and not args.no_verify and not stub:
        from oracle.pyoracle import Oracle
        nb = frame_nb
        orcs = [Oracle() for _ in range(V)]
        dpbs = [[np.full(nb + 64, fill_value, np.uint8) for _ in range(n_slots)] + [None] * (32 - n_slots) for _ in range(V)]
        for st in streams:
            for i in range(n_slots):
                st.fill(i, fill_value)
        bad = 0
        for f in range(len(packets)):
            for v in range(V):
                orcs[v].decode_frame(vpk[v][f], dpbs[v], 3)
            submit_frame(batches[f], backend.RUN_ALL)
            dev.sync()
            d = int(parsed[f].hdr["dst_slot"])
            if world == 1 and not args.no_host_packets:
                expect = expect or [[] for _ in range(V)]
                for v in range(V):
                    expect[v].append(dpbs[v][d][:nb].copy())
            for k, st in enumerate(streams):
                bad += 0 if np.array_equal(st.download(d), dpbs[k % V][d][:nb]) else 1
        verify = {"streams": len(streams), "frames_per_stream": len(packets), "frames_compared": len(streams) * len(packets), "distinct_pictures": V * len(packets),
                  "mismatching_frames": bad}
        bit_exact = bad == 0

    # ---- CPU baseline (N=1 only, the contract) -----------------------------------------------------------------------
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and not stub:
        try:
            from oracle.cpu_baseline import reference_decoder_baseline
            with launcher_cpus():
                cpu = reference_decoder_baseline(min(args.cpu_seconds, 6.0), args.cpu_seconds)
            cpu["affinity"] = "the launcher's (not the GPU's NUMA node the rank is bound to)"
        except (OSError, FileNotFoundError) as e:
            cpu = {"value": None, "unit": "frames/s", "cores": 0, "kind": "reference", "sample": f"unavailable: {e}"}
        try:  # second figure (synthetic GOP only): the reference's own sample kernels (no entropy decoding) replaying the bench packets, one core
            if args.capture:
                raise FileNotFoundError
            from oracle.pyoracle import RefKernels
            rk = RefKernels()
            nb = P.frame_bytes(W, H)
            dpb = [np.full(nb + 16, 128, np.uint8) for _ in range(n_slots)] + [None] * (32 - n_slots)
            n, tc = 0, time.perf_counter()
            while time.perf_counter() - tc < min(args.cpu_seconds, 5.0):
                for p in packets:
                    rk.replay(p, dpb, W, H, 3)
                n += len(packets)
            cpu["kernel_replay"] = {"value": round(n / (time.perf_counter() - tc), 2), "unit": "frames/s", "cores": 1,
                                    "what": "reference SSE kernels (residual + intra + inter + deblock) on the bench GOP's packets"}
        except (OSError, FileNotFoundError):
            pass

    # ---- the same GOPs out of phase (N=1 only): what a fleet of independent streams looks like to the launcher ----
    staggered = None
    if rank == 0 and world == 1 and not args.no_staggered and not stub and not args.capture and len(packets) > 1:
        staggered = staggered_leg(dev, backend, streams, dpk, vpk, groups, n_slots, fill_value, frame_nb, not args.no_verify)

    # ---- the other single-GPU configurations of BASELINE.json, short runs on the same streams (N=1 only) -----
    other = None
    if rank == 0 and world == 1 and not args.no_other_configs and not stub:
        from oracle.pyoracle import Oracle
        other = {}
        specs = [("configs[1] all-intra 4x4 I slices, residual + intra kernels only", "IIII", backend.RUN_RECON,
                  dict(i_kinds=(P.MB_I4x4,), residual_prob=1.0, deblock=False)),
                 ("configs[3] IBBP, 8x8 transform, explicit weighted bi-prediction, scaling lists, deblocking", "IPBBPBBP", backend.RUN_ALL,
                  dict(t8x8=True, scaling=True, weighted=1, num_refs=2, residual_prob=0.3, i_kinds=ALL_I))]
        for label, gop2, mode2, kw in specs:
            vpk2 = [synth.StreamSynth(W, H, seed=4321 + v, **kw).gop(gop2) for v in range(V)]  # the same number of distinct GOPs as the headline
            pk2 = vpk2[0]
            for q2 in vpk2:
                assert [int(P.Packet(q).hdr["dst_slot"]) for q in q2] == [int(P.Packet(q).hdr["dst_slot"]) for q in pk2]
            need = max(int(P.Packet(q).hdr["dst_slot"]) for q in pk2) + 1
            for st in streams:
                for i in range(n_slots, need):
                    st.alloc(i)
                for i in range(need):
                    st.fill(i, 128)
            n_slots = max(n_slots, need)
            d2 = [[dev.upload_packet(q) for q in vpk2[k % V]] for k in range(len(streams))]
            b2 = make_batches(d2)

            def step2():
                for bs in b2:
                    submit_frame(bs, mode2)
            step2()
            dev.sync()
            dev.kernel_timing(True)
            t2 = time.perf_counter()
            for _ in range(2):
                step2()
            dev.sync()
            dt2 = time.perf_counter() - t2
            k4, l4 = dev.kernel_time_ms()
            dev.kernel_timing(False)
            ok2, cmp2 = None, 0
            if not args.no_verify:  # one more GOP, untimed: EVERY stream, EVERY frame against the oracle (as the headline)
                orcs2 = [Oracle() for _ in range(V)]
                nb = P.frame_bytes(W, H)
                dpbs2 = [[np.full(nb + 16, 128, np.uint8) for _ in range(n_slots)] + [None] * (32 - n_slots) for _ in range(V)]
                for st in streams:
                    for i in range(need):
                        st.fill(i, 128)
                bad2 = 0
                for f, q in enumerate(pk2):
                    for v in range(V):
                        orcs2[v].decode_frame(vpk2[v][f], dpbs2[v], mode2)
                    submit_frame(b2[f], mode2)
                    dev.sync()
                    d = int(P.Packet(q).hdr["dst_slot"])
                    for k, st in enumerate(streams):
                        bad2 += 0 if np.array_equal(st.download(d), dpbs2[k % V][d][:nb]) else 1
                        cmp2 += 1
                ok2 = bad2 == 0
            other[label] = {"value": round(2 * len(pk2) * len(streams) / dt2, 1), "unit": "frames/s", "gop": gop2, "steps": 2, "bit_exact": ok2,
                            "frames_compared": cmp2, "distinct_pictures": V * len(pk2),
                            "kernel_ms_per_launch": {n: round(t / max(l4, 1), 4) for n, t in zip(KERNELS, k4)}}
            for b in sum(b2, []):
                dev.free_batch(b)
            for row in d2:
                for q in row:
                    q.free()

    # ---- same input on the GPU and on the CPU (N=1 only): the two 1080p bitstream fixtures ---------------------------------
    same = None
    if rank == 0 and world == 1 and not args.no_same_input and not stub and not args.capture:
        try:
            same = same_input_leg(dev, backend, my_streams, cpu)
            if cpu is not None:
                cpu["same_input"] = True  # the files of `same_input` are the files this baseline decodes
        except Exception as e:  # noqa: BLE001 -- the front-end library is built from the reference tree; without it the leg says so
            same = {"unavailable": f"{type(e).__name__}: {e}"}

    # ---- system level (N=1 only): parser + emitters + GPU on this container's cores, next to cpu_baseline (same files, same cores) ------
    system = None
    if rank == 0 and world == 1 and not args.no_system and not stub and not args.capture:
        try:
            with launcher_cpus():
                system = system_leg(cpu)
        except Exception as e:  # noqa: BLE001 -- a missing binary or a failed run is reported, never fatal for the headline
            system = {"unavailable": f"{type(e).__name__}: {e}"}

    # ---- PCIe-inclusive rate (informational, never `value`): the same GOP submitted from host memory -------------------
    pcie = None
    if rank == 0 and world == 1 and not args.no_host_packets and not stub:
        hbs = [dev.prepare_host_batch([streams[k] for k in idx], [vpk[k % V][f] for k in idx]) for f in range(len(packets)) for idx in groups]
        for hb in hbs:
            dev.submit_host_prepared(hb, backend.RUN_ALL)
        dev.sync()
        t2 = time.perf_counter()
        for _ in range(2):
            for hb in hbs:
                dev.submit_host_prepared(hb, backend.RUN_ALL)
        dev.sync()
        dt2 = time.perf_counter() - t2
        pcie = {"value": round(2 * len(packets) * len(streams) / dt2, 1), "unit": "frames/s",
                "packet_MB_per_frame": round(float(np.mean([len(p) for pk in vpk for p in pk])) / 1e6, 3),
                "what": "pageable host packets -> per-macroblock validation + copy into the batch's page-locked staging buffer by the back end's host "
                        "threads (E264_HOST_THREADS, default min(15, cores / 2)) -> ONE H2D per batch on the upload queue beside the kernels of the batch "
                        "before -> 4 kernels, asynchronous, one batch per frame index and lane"}
        # the front end's own path: packets assembled in place in page-locked memory and validated where they are produced
        for pk in vpk:
            for p in pk:
                assert backend.packet_check(p) == 0
        spins = [[dev.pinned_copy(p) for p in vpk[k % V]] for k in range(len(streams))]  # ONE page-locked buffer per stream and frame, as a front end per decoder leaves them
        pins = [pp for row in spins for pp in row]
        pbs = [dev.prepare_pinned_batch([streams[k] for k in idx], [spins[k][f] for k in idx], [len(vpk[k % V][f]) for k in idx]) for f in range(len(packets)) for idx in groups]
        for pb in pbs:
            dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        t2 = time.perf_counter()
        for _ in range(2):
            for pb in pbs:
                dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        dt2 = time.perf_counter() - t2
        pcie["pinned_in_place"] = {"value": round(2 * len(packets) * len(streams) / dt2, 1), "unit": "frames/s",
                                   "pinned_buffers": len(pins),
                                   "what": "packets already in page-locked memory (as the emitters leave them: one buffer per stream and frame) and validated by "
                                           "their producer -> gathered into the batch's staging buffer -> one H2D per batch -> 4 kernels"}
        for pp in pins:
            dev.pinned_free(pp)
        # ... and folded as e264front_set_compact(1) makes the front end fold them (the wire form, include/edge264_compact.h; the synthetic GOP gives residual to
        # nearly every macroblock and folds little -- an encoder's pictures fold to 0.7, see same_input)
        wpk = [[backend.packet_compact(p) for p in pk] for pk in vpk]
        spins = [[dev.pinned_copy(p) for p in wpk[k % V]] for k in range(len(streams))]
        pins = [pp for row in spins for pp in row]
        pbs = [dev.prepare_pinned_batch([streams[k] for k in idx], [spins[k][f] for k in idx], [len(wpk[k % V][f]) for k in idx]) for f in range(len(packets)) for idx in groups]
        for pb in pbs:
            dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        t2 = time.perf_counter()
        for _ in range(2):
            for pb in pbs:
                dev.submit_pinned_prepared(pb, backend.RUN_ALL)
        dev.sync()
        dt2 = time.perf_counter() - t2
        pcie["pinned_wire"] = {"value": round(2 * len(packets) * len(streams) / dt2, 1), "unit": "frames/s",
                               "packet_MB_per_frame": round(float(np.mean([len(p) for pk in wpk for p in pk])) / 1e6, 3),
                               "what": "pinned_in_place with the packets in their wire form (version 5): one more kernel (e264_expand_kernel) per submission, fewer bytes over the link"}
        if expect is not None:  # untimed: one more GOP from refilled slots through the wire packets, every frame of a sample of streams against the oracle's pictures
            for st in streams:
                for i in range(n_slots):
                    st.fill(i, fill_value)
            probe = sorted({0, len(streams) // 3, 2 * len(streams) // 3, len(streams) - 1})
            wbad = 0
            for f in range(len(packets)):
                for g in range(len(groups)):
                    dev.submit_pinned_prepared(pbs[f * len(groups) + g], backend.RUN_ALL)
                dev.sync()
                d = int(parsed[f].hdr["dst_slot"])
                for k in probe:
                    wbad += 0 if np.array_equal(streams[k].download(d), expect[k % V][f]) else 1
            pcie["pinned_wire"].update({"bit_exact": wbad == 0, "frames_compared": len(probe) * len(packets)})
        for pp in pins:
            dev.pinned_free(pp)
        link = link_rate_gbs()
        pcie["link_h2d_GBps_measured"] = link
        if link:
            for e in (pcie, pcie["pinned_in_place"], pcie["pinned_wire"]):
                gbs = e["value"] * pcie["packet_MB_per_frame"] * 1e6 / 1e9
                e["packet_GBps"] = round(gbs, 2)
                e["link_frac"] = round(gbs / link, 3)
            pcie["link_note"] = "link_frac = packet bytes per second / the H2D rate of one 256-MiB copy from page-locked memory on this box: near 1 = this leg is bound by the link, not by the GPU"

    single = None
    if rank == 0 and world == 1 and not args.no_single_stream and not stub and not args.capture:
        try:
            single = single_stream_leg(dev, backend, vpk[0], W, H, n_slots, frame_nb, fill_value)
        except Exception as e:  # noqa: BLE001
            single = {"unavailable": f"{type(e).__name__}: {e}"}

    rc = 0
    if rank == 0:
        L = max(launches, 1)
        kms = [t / L for t in kernel_ms4]
        own = kernel_own_bytes(models, my_streams / lanes)  # one launch = the frames of one lane's streams
        kern = {}
        for name, ms in zip(KERNELS, kms):
            sb, cb = own[name]
            g = (sb + cb) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            kern[name] = {"ms_per_launch": round(ms, 4), "sample_bytes": int(sb), "command_bytes": int(cb), "gbps": round(g, 1), "frac": round(g / HBM_PEAK_GBS, 4)}
        dom = KERNELS[int(np.argmax(kms))]
        # SURVEY 8(d) bytes of one submission: F + F x dirs (samples) + the packet (commands) per frame, x streams
        e2e_samples = float(np.mean([m["F"] * (1.0 + m["dirs"]) for m in models])) * my_streams
        e2e_cmds = float(np.mean([m["cmd_total"] for m in models])) * my_streams
        # time of one submission of ALL streams: the sum of the four launches on one lane; with several lanes the launches of
        # the groups overlap, so the wall time of the timed region per frame index is the figure
        # (the same when the parameter kernel runs on the side queue beside another kernel: its time is inside the other's)
        tot_ms = sum(kms) if lanes == 1 and not side_queue else elapsed * 1e3 / (args.steps * len(packets))
        e2e_g = (e2e_samples + e2e_cmds) / (tot_ms * 1e-3) / 1e9 if tot_ms > 0 else 0.0
        traffic, traffic_src = newest_traffic(dom, args.streams, args.gop, W, H, lanes, kms)
        sq_path, sq = newest_sq_mix(args.streams, args.gop, W, H)
        issue = issue_roofline(kern, sq_path, sq, float(np.mean([m["F"] for m in models])) * my_streams / lanes)
        dom_issue = (issue or {}).get("kernels", {}).get(dom, {}).get("valu_issue_frac")
        out = {
            "metric": "1080p frames/s/GPU (bit-exact YUV) + achieved HBM GB/s vs 8 TB/s peak",
            "value": round(value, 1), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "u8", "data": "captured bitstream packets" if args.capture else "synthetic",
            "config": {"workload": (f"{W * 16}x{H * 16} captured packets of a real bitstream ({args.gop}), one copy per stream, resident in HBM (H2D excluded, see pcie_inclusive)" if args.capture else
                                    f"{W * 16}x{H * 16} High-profile {args.gop} GOP (synthetic command packets: intra 4x4 / 8x8 / 16x16 I frame + "
                                    "P frames with 6-tap luma / bilinear chroma MC, 2 references, 4x4 and 8x8 transforms, 30% coded residual, "
                                    f"{V} distinct GOPs dealt to the streams round-robin, "
                                    "in-loop deblocking), BASELINE configs[2]; command packets and DPBs RESIDENT IN HBM before the timed region: the H2D copy of the "
                                    "packets is excluded from `value` -- see `pcie_inclusive` (host packets, copy included) and `same_input` (packets of real "
                                    "bitstreams through the reference's parser)") + (f"; configs[4]: {args.total_streams} streams sharded over {world} GPU(s)" if strong else "")
                                   + (f"; NOT the BASELINE workload: synthetic content overridden by {synth_overrides} (a measuring run)" if synth_overrides else ""),
                       "streams_per_gpu": my_streams, "total_streams": frames_per_step // len(packets), "frames_per_step": frames_per_step,
                       "waves_per_frame": args.waves, "compute_lanes": lanes, "parallelism": f"stream-parallel x{world}, no collectives",
                       "synth_overrides": synth_overrides or None},
            # `bound`: what the numbers say.  The contract's achieved / peak / frac stay the HBM figures (algorithmic bytes over the live kernel time
            # against 8 TB/s); the roof the kernels ARE under is VALU issue: `valu_issue` prices every kernel against it
            "roofline": {"bound": "valu-issue" if (dom_issue or 0) > kern[dom]["frac"] else "hbm", "kernel": dom, "achieved": kern[dom]["gbps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": kern[dom]["frac"], "traffic": traffic, "traffic_source": traffic_src,
                         "valu_issue_frac": dom_issue, "valu_issue": issue,
                         "launches": launches, "kernels": kern,
                         "end_to_end": {"ms_per_submission": round(tot_ms, 4), "sample_bytes": int(e2e_samples), "command_bytes": int(e2e_cmds),
                                        "gbps": round(e2e_g, 1), "frac": round(e2e_g / HBM_PEAK_GBS, 4)}},
            "cpu_baseline": cpu,
            "bit_exact": bit_exact, "verify": verify,
            "other_configs": other,
            "staggered_gops": staggered,
            "pcie_inclusive": pcie,
            "same_input": same,
            "system": system,
            "single_stream": single,
            "gpu_event_ms_per_step": round(ev_ms / args.steps, 3),
            "build_flags": backend.build_flags() if hasattr(backend, "build_flags") else None,
            "per_rank": {"frames_per_s": [round(r, 1) for r in rates], "min": round(min(rates), 1), "max": round(max(rates), 1),
                         "numa": numa},
        }
        os.write(json_fd, (json.dumps(out) + "\n").encode())
        if bit_exact is False or (other and any(v["bit_exact"] is False for v in other.values())) or (same and same.get("bit_exact") is False):
            print("bench.py: output is NOT bit-exact: the value above is invalid", file=sys.stderr)
            rc = 3
    for st in streams:
        st.close()
    dev.close()
    if dist is not None:
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
