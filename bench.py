#!/usr/bin/env python3
"""bench.py -- reads matched/sec of PgRC's read-to-pseudogenome matching path on MI355X.

One "step" = one full pass of the hot path over one batch: DefaultReadsMatcher::matchConstantLengthReads
(matching/ReadsMatchers.cpp:162-172) = [copMEM index build + per-read probe/verify] on the forward Pg, the
2-bit reverse complement, the same on the RC'd Pg, and the result histogram.  Inputs (2-bit packed Pg and reads)
are resident in HBM before the timed region; they are synthetic (include/pgrc_synth.h).

Workload at N=1: BASELINE.json configs[2] ("C3": 100M x 150 bp SE, mode c, seed 38, -M 50 => k<=3), the
configuration the metric is quoted on.  At N>1 every rank gets its own 100M reads (weak scaling: reads shard
with no data-path collective) and the packed Pg is shared by ONE all-gather (RCCL over xGMI) per step.
`--scaling strong` keeps the TOTAL at the workload's read count and splits it N ways (BASELINE.json configs[3], "C4":
`--workload C3-PE --scaling strong --gpus 8` = 100M PE reads over 8 GPUs); every rank still builds the whole index.

Prints ONE JSON line on rank 0 with `roofline` and `phases_ms` (figures of the timed steps themselves).  A plain run does only
what that line's headline needs: set up, warm up, time the steps, write `--dump-outputs`, print.  `--full` adds the legs that take
runs of their own: `cpu_baseline` (the reference on the host cores), `parity_sample` (a sample checked against the reference)
and, for C3 / C3-N, `boundary` (the same job from host buffers through the C ABI).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (reads per GPU, read_len, pg_len, seed_len, min_chars_per_mismatch, mode, paired)
    "C3": (100_000_000, 150, 1_875_000_000, 38, 50, "c", False),
    "C2": (10_000_000, 100, 125_000_000, 38, 50, "c", False),
    "C3-PE": (100_000_000, 150, 1_875_000_000, 38, 50, "c", True),
    "C5-shard": (62_500_000, 250, 3_100_000_000, 38, 50, "c", False),  # one GPU's 1/8 of configs[4]
    "P64": (50_000_000, 150, 4_400_000_000, 38, 50, "c", False),  # Pg >= 4 Gi: the 64-bit-position kernels
    "tiny": (1_000_000, 150, 18_750_000, 38, 50, "c", False),
    # C3 as the encoder really submits it (pgrc-encoder.cpp:349-352): the LQ set followed by the N set -- 98 M ACGT reads +
    # 2 M reads holding 1-3 'N' (the generator's last reads), handed over in the reference's two packings before the timed region
    "C3-N": (100_000_000, 150, 1_875_000_000, 38, 50, "c", False),
    # C3 at PgRC's shipped mismatch limit (-M 3: k <= L / 3 = 50, pgrc-params.h:138-146)
    "C3-M3": (100_000_000, 150, 1_875_000_000, 38, 3, "c", False),
    "tiny-N": (1_000_000, 150, 18_750_000, 38, 50, "c", False),
    # rows a5-a7: the reference's other matchers at the C3 size (ReadsMatchers.cpp:715-740: mode d / i with seed 38, the exact
    # matcher when the seed is the whole read); seedidx.hip.  M = 3 as tools/modes_c3.py has it (k <= 3 = parts - 1)
    "C3-d": (100_000_000, 150, 1_875_000_000, 38, 50, "d", False),
    "C3-i": (100_000_000, 150, 1_875_000_000, 38, 50, "i", False),
    "C3-e": (100_000_000, 150, 1_875_000_000, 150, 50, "e", False),
    "tiny-d": (1_000_000, 150, 18_750_000, 38, 50, "d", False),
    # short reads (few seeds per read): where the dual kernel's schedule stops paying (tools/ab_match.py, PGRC_DUAL=0 / 1)
    "S75": (10_000_000, 75, 125_000_000, 38, 25, "c", False),
    "S50": (10_000_000, 50, 125_000_000, 38, 25, "c", False),
}
N_FRACTION = {"C3-N": 0.02, "tiny-N": 0.02}     # share of the reads that hold an N (the reference's N read set)
# measured random-request ceiling of the chip (tools/ubench/gather.hip): 51 G/s at a 4 GiB footprint, 48 G/s at the
# 8-32 GiB footprints where the bucket-head table of C3 lives (profiles/r01_ubench_gather_footprint.txt); the unit of a
# request is a 128-BYTE line (round 4, profiles/r04_head_interleave_ab.txt): two 16-byte loads of one lane into one such
# line cost 1.2 requests (41 G lines/s with two loads per line, profiles/r01_ubench_gather_same_line.txt)
GATHER_CEILING_GPS = 48.0
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default=os.environ.get("PGRC_BENCH_WORKLOAD", "C3"), choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the CPU baseline, the parity sample and the boundary leg (the --no-* / --cpu-* / "
                         "--parity-* options below shape them); off by default: a plain run only sets up, warms up, times the steps, "
                         "dumps and prints")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline's main leg (0 = all of the box's hardware threads: BASELINE.md section 3, `-t $(nproc)`)")
    ap.add_argument("--no-boundary", action="store_true", help="with --full: skip the boundary leg (host buffers -> host results through the C ABI, PCIe included; never `value`)")
    ap.add_argument("--no-cpu-t1", action="store_true", help="skip the -t 1 leg of the CPU baseline (two more serial index builds)")
    ap.add_argument("--cpu-sample-reads", type=int, default=3_000_000)
    ap.add_argument("--parity-sample-reads", type=int, default=100_000,
                    help="with --full: reads checked bit for bit against the SERIAL-index reference (0 = skip)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: the workload's reads PER GPU (default, the driver's contract); strong: that many reads in TOTAL, split over the GPUs")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo + PGRC_BENCH_FORCE_DEVICE=0 rehearses the N>1 path on a one-GPU box (collectives staged through the host)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rank 0's results) as DIR/<name>.npy; see dump_outputs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import numpy as np
    import torch
    import torch.distributed as dist

    from pgrc_amd import MatchContext, copmem_params, synth
    from pgrc_amd import dist as pdist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    if "PGRC_BENCH_FORCE_DEVICE" in os.environ:
        local_rank = int(os.environ["PGRC_BENCH_FORCE_DEVICE"])
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    n_work, L, G, seed_len, M, mode, paired = WORKLOADS[args.workload]
    if args.scaling == "strong" and world > 1:
        # contiguous, even-aligned shares of ONE read set (PE mates stay together: ReadsMatchers.cpp:553)
        lo, hi = pdist.shard_range(n_work, rank, world)
        n_per, first_read, n_total = hi - lo, lo, n_work
    else:
        n_per, first_read, n_total = n_work, rank * n_work, n_work * world
    kmax = L // M
    nw = (L + 15) // 16
    stride = (n_per + 63) & ~63
    pg_words = (G + 15) // 16

    # ---- inputs straight into HBM
    g = synth.pg_params(G, seed=12345)
    nfrac = N_FRACTION.get(args.workload, 0.0)
    if nfrac:
        # the LQ + N sum set: made on the device, brought to the host in the reference's two packings (tools/boundary_c3.py)
        # and handed over through the boundary BEFORE the timed region -- the library keeps the N rows in its side list
        if world > 1:
            raise SystemExit("the workloads with N reads are single-GPU lines")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import boundary_c3
        pg_host, lq_rows, n_rows, n_lq, n_n = boundary_c3.make_host_inputs(n_per, L, G, nfrac)
        rs = synth.reads_params(n_total, L, seed=12345, paired=paired, n_with_n=n_n)
        _TEXT[G] = pg_host
        ctx = MatchContext(L, seed_len, kmax, 0, mode, device=local_rank)
        ctx.set_pg_ascii(pg_host)
        ctx.set_reads_packed_sets([(lq_rows, n_lq, 4), (n_rows, n_n, 5)])
        ctx._host_rows = (lq_rows, n_lq, n_rows, n_n)
        ctx.set_profiling(True)
        d_pg = None
    else:
        rs = synth.reads_params(n_total, L, seed=12345, paired=paired)
        d_pg = torch.zeros(pg_words + 64, dtype=torch.int32, device=dev)
        synth.pg_device(g, d_pg.data_ptr())
        d_reads = torch.empty(nw * stride, dtype=torch.int32, device=dev)
        synth.reads_device(g, d_pg.data_ptr(), rs, first_read, n_per, d_reads.data_ptr(), stride)
        torch.cuda.synchronize()

        ctx = MatchContext(L, seed_len, kmax, 0, mode, device=local_rank)
        ctx.set_reads_device(d_reads.data_ptr(), n_per, stride, keep=d_reads)
        ctx._keep_reads = d_reads
        ctx.set_profiling(True)

    # multi-GPU: every rank owns 1/world of the packed Pg (what it would pack from its slice of the host text);
    # one all-gather per step rebuilds the replicated text
    if world > 1:
        slo, shi, slice_words = pdist.pg_slice(G, rank, world)     # the symbols this rank packs: words [lo/16, ...)
        d_slice = torch.zeros(slice_words, dtype=torch.int32, device=dev)
        wlo, whi = slo // 16, (shi + 15) // 16
        if whi > wlo:
            d_slice[: whi - wlo] = d_pg[wlo:whi]
        del d_pg
    elif d_pg is not None:
        ctx.set_pg_packed_device(d_pg.data_ptr(), G)
        ctx._pg_ptr, ctx._pg_keep = d_pg.data_ptr(), d_pg

    ag_ms = []                        # per step: the all-gather (this rank's clock, the stream drained on both sides)

    def step():
        if world > 1:
            # the ONE data-path collective: all-gather of the packed text (RCCL over xGMI; pgrc_amd/dist.py)
            ta = time.perf_counter()
            d_full = pdist.all_gather_packed_pg(d_slice, world)
            torch.cuda.current_stream().synchronize()
            ag_ms.append((time.perf_counter() - ta) * 1e3)
            ctx.set_pg_packed_device(d_full.data_ptr(), G)
        ctx.init_results()
        ctx.run(True)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    sync()
    del ag_ms[:]
    step_ms = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        step()                        # (synchronous: pgrc_match_run returns when the histogram of the results is on the host)
        step_ms.append((time.perf_counter() - ts) * 1e3)
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(ctx, args.dump_outputs)
    _, _, _, hist, matched = ctx.get_results(arrays=False)
    ctr = ctx.counters()
    cp = copmem_params(seed_len, G)
    # N > 1: what every rank spent where (the driver's SCALE record is one number per N: this makes it readable) -- the last
    # step's device phases, the all-gather per step (mean), the rank's own clock over its K steps
    per_rank = None
    if world > 1:
        mine = {"rank": rank, "reads": n_per, "ms_per_step": sum(step_ms) / max(len(step_ms), 1), "allgather_ms": sum(ag_ms) / max(len(ag_ms), 1),
                "index_ms": ctr["ms_index"][0] + ctr["ms_index"][1], "match_ms": ctr["ms_screen"] + ctr["ms_match"][0] + ctr["ms_match"][1],
                "other_ms": ctr["ms_other"], "total_device_ms": ctr["ms_total"], "matched": int(matched)}
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        per_rank = gathered

    if rank == 0:
        total_reads = n_total * args.steps
        value = total_reads / dt
        step_sorted = sorted(step_ms)
        if mode != "c":
            print(json.dumps(seed_mode_line(args, ctx, ctr, value, dt, step_sorted, world, n_per, n_total, L, G, seed_len, kmax, mode, matched)), flush=True)
            if world > 1:
                dist.barrier()
                dist.destroy_process_group()
            return
        # ---- roofline of the dominant kernel: the forward-pass match kernel (k_copmem_match)
        # algorithmic bytes: per searched read its packed words and
        # the 10-B result; per executed seed probe one 8-B bucket range; per verified candidate a 4-B position
        # and the (L/4 + 1)-B text window.
        rb = (L + 3) // 4
        schedule = {0: "two passes", 1: "screened", 2: "dual"}[ctr["screened"]]
        dom = 0 if ctr["ms_match"][0] >= ctr["ms_match"][1] else 1
        if schedule == "dual":
            # one launch does a read's query over both strands; the two ordinary passes after it only see
            # the reads it left undecided: the dual kernel is the dominant one
            kc = ctr["dual"]
            ms = ctr["ms_screen"]
            kname = "k_copmem_match_dual"
        else:
            kc = {k: ctr[k][dom] for k in ("searched", "probes", "candidates", "entry_fetches", "verifies")}
            ms = ctr["ms_match"][dom]
            kname = "k_copmem_match" + ("(fwd)" if dom == 0 else "(rc)")
        alg_bytes = kc["searched"] * (rb + 10) + kc["probes"] * 8 + kc["candidates"] * (5 + rb)
        achieved = alg_bytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        # random line requests issued by that launch: one per probed SEED under the pair table (round 4: a seed's forward and RC
        # head share a 128-byte line; `dual_seed_probes`) -- one per probed head otherwise --, one per fetched entry pair, and
        # per verified text window the 128-byte lines a (L/4)-byte window at a random 4-B offset spans on average
        # (tools/ubench: the chip sustains ~48-51 G independent random requests per second, whatever their width)
        head_lines = ctr.get("dual_seed_probes", 0) if (schedule == "dual" and ctr.get("dual_seed_probes", 0)) else kc["probes"]
        gathers = int(head_lines + kc["entry_fetches"] + kc["verifies"] * (1.0 + max(rb - 4, 0) / 128.0))
        gather_rate = gathers / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        # the bytes THIS kernel's algorithm needs (its fingerprints reject 99.9 % of the false candidates without
        # touching the text, so the reference's text-window bytes above are mostly never moved): a 16-B head per
        # probe, 16 B per fetched entry pair, a window only per VERIFIED candidate, the read and the result
        kernel_bytes = kc["probes"] * 16 + kc["entry_fetches"] * 16 + kc["verifies"] * (5 + rb) + kc["searched"] * (rb + 10)
        kernel_gbs = kernel_bytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        # HBM traffic of that launch from the PMC counters (FETCH_SIZE + WRITE_SIZE): they cannot be read from inside
        # this process, so the value comes from the committed separate `rocprofv3 --pmc` passes of this very command
        # (tools/pmc_groups.sh + tools/pmc_traffic.py -> profiles/); null for workloads that were not profiled.
        traffic, traffic_src, index_traffic = None, None, None
        for rnd in ("r05", "r04", "r03", "r02", "r01_final"):
            tp = os.path.join(ROOT, "profiles", f"{rnd}_{args.workload.lower()}_traffic.json")
            if os.path.exists(tp):
                break
        if world == 1 and os.path.exists(tp):
            try:
                tj = json.load(open(tp))
                # the profile names the schedule it was taken under and lists that step's match launches in order:
                # "two passes": fwd, rc; "screened": screen, fwd, rc; "dual": dual kernel, fwd, rc (the two redo passes)
                if tj.get("schedule", "two passes") != schedule:
                    raise KeyError("profile taken under another schedule")
                dsp = tj["dispatches"][0 if schedule == "dual" else dom + (1 if schedule == "screened" else 0)]
                # HBM bytes: every read request of the L2 is a 128-BYTE line that FETCH_SIZE tallies at 64 (calibrated in round 5
                # on random gathers: profiles/r05_ubench_gather_pmc.txt) -- profiles of earlier rounds stored the raw FETCH_SIZE
                traffic = dsp["hbm_bytes"] if "unit_note" in tj else 2.0 * dsp["fetch_bytes"] + dsp["write_bytes"]
                traffic_src = os.path.relpath(tp, ROOT)
                ips = tj.get("index_per_strand", {})
                index_traffic = ips.get("hbm_bytes")
                if index_traffic and "unit_note" not in tj:
                    index_traffic = None                      # (an older round's build: not this one's bytes)
            except Exception:
                traffic = None
        out = {
            "metric": "reads matched/sec (150 bp) at 1/2/4/8 MI355X; achieved HBM GB/s",
            "value": value,
            "unit": "reads/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "ms_per_step_min_median_max": [step_sorted[0], step_sorted[len(step_sorted) // 2], step_sorted[-1]],   # rank 0's steps
            "higher_is_better": True,
            "scaling": args.scaling if world > 1 else "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {"workload": (f"{args.workload}: {n_per} x {L} bp {'PE' if paired else 'SE'} reads per GPU" if not (args.scaling == "strong" and world > 1) else
                                    f"{args.workload} (strong scaling): {n_total} x {L} bp {'PE' if paired else 'SE'} reads in total, split over {world} GPUs,")
                                   + f" vs Pg of {G} bp, mode {mode}, seed {seed_len}, -M {M} (k<={kmax}), both strands",
                       "symbols": "2-bit packed, 16 per u32 word (integer xor/popcount work, no floating point)",
                       "reads_with_N": int(getattr(ctx, "_host_rows", (0, 0, 0, 0))[3]),
                       "reads_per_gpu": n_per, "read_len": L, "pg_len": G, "seed_len": seed_len, "max_mismatches": kmax,
                       "copmem": cp, "matched_fraction": matched / n_per,
                       "parallelism": f"reads sharded x{world}, Pg replicated" + (" (1 all-gather/step)" if world > 1 else "")},
            # `bound` keeps to the two values the bench contract knows: the kernel is priced against the HBM byte roofline
            # (`frac`, SURVEY 8d bytes).  What it actually runs into is named in `binding_limit`: its memory waits -- random 128-B
            # line requests at 0.77 of the rate the chip serves them (`gather_frac`), one per lane in flight (profiles/r05_dual_sq_counters.txt).
            "roofline": {"bound": "hbm", "binding_limit": "memory waits: random 128-B line requests (a 16-byte head costs a line), one per lane in flight at six waves per SIMD; waves wait for a memory counter 59 % of their time, VALU issue 78 % busy (profiles/r05_dual_sq_counters.txt)",
                         "index": dict(index_roofline(ctr, cp, G, n_strands=2), traffic=(2 * index_traffic if index_traffic else None),
                                       traffic_note="HBM bytes of both strands' builds from the same committed PMC passes as `traffic`"),
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_unit": "HBM bytes per launch = 2 x FETCH_SIZE + WRITE_SIZE: a TCC_EA0_RDREQ is a 128-byte line on gfx950, for random 16-byte gathers as for streams (profiles/r05_ubench_gather_pmc.txt)",
                         "traffic_GBps": (traffic / (ms * 1e-3) / 1e9 if traffic and ms > 0 else None),
                         "kernel": kname, "schedule": schedule,
                         "kernel_ms": ms, "algorithmic_bytes": alg_bytes,
                         # every launch of the match kernel in a step (the screened schedule has three: screen, forward
                         # pass, RC pass) and their mean -- what `rocprofv3 --stats` reports as the kernel's average
                         "match_launches_ms": ([ctr["ms_screen"]] if ctr["screened"] else []) + list(ctr["ms_match"]),   # (screen or dual kernel first)
                         "match_launches_mean_ms": (ctr["ms_screen"] + sum(ctr["ms_match"])) / (3 if ctr["screened"] else 2),
                         "kernel_bytes": kernel_bytes, "achieved_kernel_bytes": kernel_gbs,
                         "frac_kernel_bytes": kernel_gbs / HBM_PEAK_GBS,
                         "limiter": "random accesses (one per probed seed -- its two heads share a 128-B line --, entry pair, text window): each costs a 128-byte line; the chip serves ~49 G random lines/s (54 G/s with the non-temporal hint, tools/ubench/gather_modes.hip); the kernel asks for ~38 G/s with one request per lane in flight, its waves waiting for memory 59 % of the time and its SIMDs issuing VALU instructions 78 % of the time (27-33 % of the lanes active in an average instruction): DESIGN.md 4.2",
                         "head_line_requests": int(head_lines), "heads_probed": int(kc["probes"]),
                         "random_gathers": gathers, "gather_rate_G_per_s": gather_rate,
                         "gather_ceiling_G_per_s": GATHER_CEILING_GPS, "gather_frac": gather_rate / GATHER_CEILING_GPS},
            "phases_ms": {"index_fwd": ctr["ms_index"][0], "match_fwd": ctr["ms_match"][0], "index_rc": ctr["ms_index"][1],
                          "match_rc": ctr["ms_match"][1], "other": ctr["ms_other"], "total_device": ctr["ms_total"],
                          # the screened schedule: both indexes first, then an exact-match screen on the RC
                          # text, the forward pass, the RC pass; "screen" is that first launch (0 when the run did not take it)
                          "screen": ctr["ms_screen"], "screened_schedule": bool(ctr["screened"]), "schedule": schedule,
                          "schedule_note": {"dual": "'screen' is the dual kernel (every read, both strands at once); match_fwd / match_rc are the two ordinary passes over the reads it left undecided",
                                            "screened": "'screen' = exact-match screen on the RC text, then the forward and the RC pass",
                                            "two passes": None}[schedule],
                          "index_note": ("both index builds run at once on two streams: index_fwd is the pair, index_rc ~ 0"
                                         if ctr["screened"] and ctr["ms_index"][1] < 0.1 * ctr["ms_index"][0] else None)},
            "dist_backend": args.dist_backend if world > 1 else None,
            "allgather_ms": (sum(ag_ms) / max(len(ag_ms), 1) if world > 1 else None),       # rank 0's mean per step (inside the timed region)
            "ranks": per_rank,
            "counters": {k: ctr[k] for k in ("searched", "candidates", "probes", "entry_fetches", "verifies", "index_entries", "dual", "redo_reads", "dual_seed_probes")},
        }
        # ---- the legs of --full: runs of their own after the timed steps, never `value`
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args, ctx, g, rs, n_per, L, G, seed_len, kmax)
            except Exception as e:  # the GPU measurement must not be lost to a host-side problem
                out["cpu_baseline"] = {"value": None, "unit": "reads/s", "cores": 0, "kind": "port", "sample": "failed: " + repr(e)}

        if args.full and args.parity_sample_reads > 0:          # (at N > 1: rank 0's shard -- its own reads, the gathered text it matched them against)
            try:
                out["parity_sample"] = parity_sample(args, ctx, g, rs, n_per, L, G, seed_len, kmax)
                if world > 1:
                    out["parity_sample"]["shard"] = f"rank 0 of {world}: reads [{first_read}, {first_read + n_per}) of the set"
            except Exception as e:
                out["parity_sample"] = {"diff": None, "error": repr(e)}
        if args.full and world == 1 and not args.no_boundary and args.workload in ("C3", "C3-N"):
            try:
                out["boundary"] = boundary_leg(n_per, L, G, kmax)
            except Exception as e:
                out["boundary"] = {"reads_per_s": None, "error": repr(e)}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


DUMP_SAMPLE_READS = 1 << 20     # at most this many reads' results are dumped: 24 MB of .npy files
DUMP_SAMPLE_SEED = 20240607


def dump_outputs(ctx, out_dir):
    """What the timed path hands its caller after the last step (pgrc_match_get_results: per read its position, RC flag and
    mismatch count, the histogram of the mismatch counts, the number of matched reads), written as .npy for an output-for-output
    comparison of two builds.  Above DUMP_SAMPLE_READS reads, a fixed seeded sample of the reads (the same for every run of a
    workload; `read_index` names them).  Positions go to float64 (exact below 2^53; the unmatched value 2^64 - 1 rounds to 2^64)."""
    import numpy as np
    pos, rc, mism, hist, matched = ctx.get_results()
    n = pos.size
    if n > DUMP_SAMPLE_READS:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, DUMP_SAMPLE_READS, replace=False))
    else:
        idx = np.arange(n)
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"read_index": idx.astype(np.float64), "pos": pos[idx].astype(np.float64), "rc": rc[idx].astype(np.float32),
              "mism": mism[idx].astype(np.float32), "hist": hist.astype(np.float64), "matched": np.array([matched], dtype=np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def boundary_leg(n, L, G, kmax):
    """What a PgRC process pays at the drop-in boundary (never `value`): the encoder's call site hands over a finished pseudogenome
    as ASCII and the LQ + N sum set in the reference's two packings, all in HOST memory, and wants the three result vectors back
    in host memory (pgrc-encoder.cpp:342-374 -> mapReadsIntoPg -> matchConstantLengthReads, matching/ReadsMatchers.cpp:162-172,
    :421-451).  Timed from context creation to the arrays on the host, through pgrc_match_set_pg_ascii / _prepare_index /
    _stream_begin / _append_reads_packed / _stream_end (the pipelined hand-over, pgrc_amd/csrc/stream.hip) and, for comparison,
    with the steps in turn; PCIe included.  One throw-away job first (first allocations, code object load).  Outside the timed
    loop, like cpu_baseline."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import boundary_c3
    from pgrc_amd import MatchContext
    t0 = time.perf_counter()
    pg, lq_rows, n_rows, n_lq, n_n = boundary_c3.make_host_inputs(n, L, G, 0.02)
    prep_s = time.perf_counter() - t0
    sets = [(lq_rows, n_lq, 4), (n_rows, n_n, 5)]
    res = (np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8))
    for r_ in res:
        r_ += 0
    up_bytes = int(pg.nbytes + lq_rows.nbytes + n_rows.nbytes)
    down_bytes = n * 10
    # the link itself: pinned 1 GiB copies each way (what tools/ubench/pcie.hip measures)
    pin = torch.empty(1 << 30, dtype=torch.uint8).pin_memory()
    dev = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    link = {}
    for name, (src, dst) in (("h2d", (pin, dev)), ("d2h", (dev, pin))):
        dst.copy_(src, non_blocking=True); torch.cuda.synchronize()
        t = time.perf_counter(); dst.copy_(src, non_blocking=True); torch.cuda.synchronize()
        link[name] = (1 << 30) / (time.perf_counter() - t) / 1e9
    del pin, dev
    warm = MatchContext(L, 38, kmax, 0, "c"); warm.set_pg_ascii(pg); warm.set_reads_packed_sets(sets); warm.init_results(); warm.run(True)
    warm.get_results(out=res)
    ref = tuple(a.copy() for a in res)
    del warm
    legs = {}
    for leg in ("pipelined", "in_turn"):
        best = None
        for rep_ in range(2):
            t = time.perf_counter()
            ctx = MatchContext(L, 38, kmax, 0, "c"); ctx.set_pg_ascii(pg)
            if leg == "pipelined":
                ctx.prepare_index(True)
                pos, rc, mism, hist, matched = ctx.match_streamed(sets, out=res)
            else:
                ctx.set_reads_packed_sets(sets); ctx.init_results(); ctx.run(True)
                pos, rc, mism, hist, matched = ctx.get_results(out=res)
            dt = time.perf_counter() - t
            same = bool(np.array_equal(pos, ref[0]) and np.array_equal(rc, ref[1]) and np.array_equal(mism, ref[2]))
            del ctx
            if best is None or dt < best[0]:
                best = (dt, same, int(matched))
        legs[leg] = {"s": best[0], "reads_per_s": n / best[0], "same_results": best[1]}
    pl = legs["pipelined"]
    link_bound_s = up_bytes / (link["h2d"] * 1e9) + down_bytes / (link["d2h"] * 1e9)
    return {"what": "C3-N through the C ABI from HOST buffers (ASCII text, the reference's packed LQ + N rows) to the three result vectors on the host; PCIe included; best of two jobs after a throw-away one",
            "reads_per_s": pl["reads_per_s"], "s": pl["s"], "same_results_as_in_turn": pl["same_results"] and legs["in_turn"]["same_results"],
            "in_turn": legs["in_turn"], "up_bytes": up_bytes, "down_bytes": down_bytes,
            "up_GBps": up_bytes / pl["s"] / 1e9, "down_GBps": down_bytes / pl["s"] / 1e9,
            "link_GBps": link, "link_bound_s": link_bound_s, "link_bound_reads_per_s": n / link_bound_s,
            "frac_of_link_bound": link_bound_s / pl["s"], "prep_s": prep_s}


def seed_mode_line(args, ctx, ctr, value, dt, step_sorted, world, n_per, n_total, L, G, seed_len, kmax, mode, matched):
    """The bench line of the workloads in modes d / i / e (rows a5-a7, seedidx.hip).  Algorithmic bytes counted SURVEY-8d style (ONE
    formula, the one tools/modes_c3.py prints): per window start and strand one 8-byte table key; per (window, part) pair with equal
    keys -- a hit -- the entry (4 B), the read's and the window's L symbols at 2 bits and the read's 8-byte key; per read its packed
    words and its three result fields.  `hits` are those of the LAST run (pgrc_match_run clears the counters when it starts).  What
    the path runs into is the same as in mode c: random line requests (one per window probe, about three per hit), not bytes."""
    import zlib
    import numpy as np
    P = 1 if mode == "e" else L // seed_len
    nw = (L + 15) // 16
    nwin = G - (L if mode == "e" else seed_len * (P if mode == "i" else 1)) + 1
    hits = ctr["candidates"][0] + ctr["candidates"][1]
    alg = 2 * nwin * 8 + hits * (4 + 2 * ((L + 3) // 4) + 8) + n_per * (4 * nw + 10)
    ms = dt / args.steps * 1e3
    pos, rc, mism, _, _ = ctx.get_results()
    digest = "%08x-%08x-%08x" % (zlib.crc32(pos.data), zlib.crc32(rc.data), zlib.crc32(mism.data))
    req = 2 * nwin + 3 * hits + n_per * P
    traffic = None
    tp = os.path.join(ROOT, "profiles", f"r05_{args.workload.lower()}_traffic.json")
    if os.path.exists(tp):
        try:
            traffic = json.load(open(tp)).get("hbm_bytes_per_step")
        except Exception:
            traffic = None
    out = {"metric": "reads matched/sec (150 bp) at 1/2/4/8 MI355X; achieved HBM GB/s", "value": value, "unit": "reads/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "ms_per_step_min_median_max": [step_sorted[0], step_sorted[len(step_sorted) // 2], step_sorted[-1]],
           "higher_is_better": True, "scaling": args.scaling if world > 1 else "weak", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
           "config": {"workload": f"{args.workload}: {n_per} x {L} bp SE reads per GPU vs Pg of {G} bp, mode {mode} (parts of {seed_len} symbols, k<={kmax}), both strands",
                      "symbols": "2-bit packed, 16 per u32 word (integer xor/popcount work, no floating point)",
                      "reads_per_gpu": n_per, "read_len": L, "pg_len": G, "seed_len": seed_len, "max_mismatches": kmax, "matched_fraction": matched / n_per,
                      "parallelism": f"reads sharded x{world}, Pg replicated"},
           "roofline": {"bound": "hbm", "binding_limit": "random line requests: one per window start of the forward text (both strands in one scan), about three per hit",
                        "achieved": alg / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": traffic,
                        "traffic_source": (os.path.relpath(tp, ROOT) if traffic else None),
                        "kernel": "k_seed_probe + k_seed_expand + k_seed_heavy (seedidx.hip)", "kernel_ms": ctr["ms_total"], "kernel_ms_note": "device time of the whole run (HIP events), host waits between batches included",
                        "algorithmic_bytes": alg, "algorithmic_bytes_formula": "2 strands x windows x 8 + hits x (4 + 2 x ceil(L/4) + 8) + reads x (4 x words + 10)",
                        "windows": nwin, "hits_per_step": hits,
                        "random_requests_ESTIMATE": req, "gather_rate_G_per_s_ESTIMATE": req / (ms * 1e-3) / 1e9, "estimate_note": "2 per window start + 3 per hit + 1 per (read, part): a model, not a counter",
                        "gather_ceiling_G_per_s": GATHER_CEILING_GPS},
           "counters": {"searched": ctr["searched"], "candidates": ctr["candidates"]},
           "results_digest": digest}
    if args.full and world == 1 and args.parity_sample_reads > 0:
        try:
            out["parity_sample"] = seed_parity_sample(args, ctx, n_per, L, G, seed_len, kmax, mode)
        except Exception as e:
            out["parity_sample"] = {"diff": None, "error": repr(e)}
    if args.full and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = seed_cpu_baseline(n_per, L, G, seed_len, kmax, mode)
        except Exception as e:
            out["cpu_baseline"] = {"value": None, "unit": "reads/s", "cores": 0, "kind": "reference", "sample": "failed: " + repr(e)}
    return out


def seed_parity_sample(args, ctx, n_per, L, G, seed_len, kmax, mode):
    """Bit-parity inside the bench line of modes d / i / e: the first reads of the workload matched ALONE against the whole text on the
    GPU (a second context over the same device buffers: in these modes the candidates depend on which reads are indexed together) and by
    the oracle's serial scan of the whole text (tests/oracle.py: the reference's DefaultReadsApproxMatcher /
    InterleavedReadsApproxMatcher / DefaultReadsExactMatcher::executeMatching, matching/ReadsMatchers.cpp:198-230, :297-409, restated;
    about 80 s on one core at the C3 text) -- results AND the number of hits per strand."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc
    from pgrc_amd import MatchContext
    ns = min(args.parity_sample_reads, 20_000, n_per)
    nw, stride = (L + 15) // 16, (n_per + 63) & ~63
    idx = np.arange(ns, dtype=np.int64)
    reads = reads_from_hbm(ctx._keep_reads, idx, nw, stride, L)
    pg = host_text(ctx, G)
    cx = MatchContext(L, seed_len, kmax, 0, mode)
    cx.set_pg_packed_device(ctx._pg_ptr, G)
    cx.set_reads_device(ctx._keep_reads.data_ptr(), ns, stride, keep=ctx._keep_reads)
    cx.init_results()
    cx.run(True)
    pos, rc, mism, _, _ = cx.get_results()
    cand = cx.counters()["candidates"]
    del cx
    t = time.perf_counter()
    o = orc.oracle_match(mode, pg, reads, seed_len, kmax, 0, True, 1)
    secs = time.perf_counter() - t
    d_pos, d_rc, d_mism = int((pos != o["pos"]).sum()), int((rc != o["rc"]).sum()), int((mism != o["mism"]).sum())
    d_cand = int(int(cand[0]) != int(o["candidates"][0])) + int(int(cand[1]) != int(o["candidates"][1]))
    return {"reads": ns, "drawn": f"the first {ns} reads of the workload, matched alone against the whole {G}-bp text", "checker": "oracle port (serial scan of the whole text)",
            "diff": d_pos + d_rc + d_mism + d_cand, "diff_pos": d_pos, "diff_rc": d_rc, "diff_mism": d_mism,
            "hits_gpu": [int(v) for v in cand], "hits_checker": [int(v) for v in o["candidates"]],
            "matched_in_sample": int((o["mism"] != 255).sum()), "checker_s": secs}


def seed_cpu_baseline(n_per, L, G, seed_len, kmax, mode, scale=50):
    """The reference's matcher of this mode on the host, one thread (the code is serial: ConstantLengthPatternsOnTextHashMatcher +
    ReadsMatchers.cpp:198-230, :297-409).  Its scan of the whole text would take minutes, so the leg is a SCALED-DOWN INSTANCE of the
    same workload at the same read density: a text of G / 50 symbols from the same generator and n / 50 reads drawn from it.  The rate
    is that instance's, not an extrapolation; the real instance's hash table is 50 times larger (more cache misses per probe), so the
    reference is slower than this on the full job."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc
    from pgrc_amd import synth
    Gs, ns = G // scale, n_per // scale
    g = synth.pg_params(Gs, seed=12345)
    pg = synth.pg_host(g)
    rs = synth.reads_params(ns, L, seed=12345)
    reads = synth.reads_host(g, pg, rs, 0, ns)
    kind = "reference" if orc.have_ref() else "port"
    t = time.perf_counter()
    if kind == "reference":
        r = orc.ref_match(mode, pg, reads, seed_len, kmax, 0, True, 0, 1, 1)
    else:
        r = orc.oracle_match(mode, pg, reads, seed_len, kmax, 0, True, 1)
    secs = time.perf_counter() - t
    return {"value": ns / secs, "unit": "reads/s", "cores": 1, "nproc": os.cpu_count(), "kind": kind, "extrapolated": False,
            "sample": f"a 1/{scale} instance of the workload at the same read density: {ns} x {L} bp reads against a {Gs}-bp text of the same generator, both strands, "
                      f"one thread (the reference's matcher of mode {mode} is serial): {secs:.1f} s; the full instance's table is {scale} x larger, so its rate is lower",
            "matched_in_sample": int((r["mism"] != 255).sum())}


def index_roofline(ctr, cp, G, n_strands):
    """the second-largest phase: both strands' index builds (they run at once on two streams).  Algorithmic bytes per
    strand as SURVEY 8d prices them: G/4 of packed text read, 4 B per sampled position and 4 B per bucket written."""
    npos = (G - cp["K"]) // cp["k1"] + 1 if G >= cp["K"] else 0
    alg = n_strands * (G // 4 + npos * 4 + cp["hash_size"] * 4)
    # what THIS build writes at least (16-B bucket heads, 8-B entries of buckets of three or more ~ 16 % of the samples)
    ms = ctr["ms_index"][0] + ctr["ms_index"][1]
    gbs = alg / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    own = n_strands * (G // 4 + cp["hash_size"] * 16)
    return {"ms": ms, "strands": n_strands, "algorithmic_bytes": alg, "achieved": gbs, "frac": gbs / HBM_PEAK_GBS,
            "own_output_bytes": own, "frac_own_output": own / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS if ms > 0 else 0.0,
            "kernels": "k_os_count_gen, k_os_scatter_gen, k_os_count_bins, k_os_scatter_bins (idxsweep.hip), k_ps_finish_fast (idxsort.hip)"}


def unpack_pg_to_ascii(words):
    import numpy as np
    lut = np.zeros((256, 4), dtype=np.uint8)
    for b in range(256):
        for k in range(4):
            lut[b, k] = b"ACGT"[(b >> (2 * k)) & 3]
    return lut[words.view(np.uint8)].reshape(-1)


def cpu_baseline(args, ctx, g, rs, n_per, L, G, seed_len, kmax):
    """The CPU path timed on this box's host cores, on a bounded sample: the WHOLE pseudogenome (so index size and
    cache behaviour are the real ones) and the first `cpu_sample_reads` reads of the same read set.  Whole-job
    rate for the full read set is extrapolated from two runs (fixed cost a = 2 index builds + RC sweeps, slope b
    per read):  value = N / (a + b*N).  kind "reference" = the real PgRC code (oracle/_ref); "port" = oracle/.
    Three legs, as BASELINE.md section 3 asks: `-t $(nproc)` (the main value: BASELINE.json configs[1] says "CPU -t all"),
    `-t 16` (what rounds 1-4 reported) and `-t 1` (serial index build, one thread in the per-read loop: the parity target)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc
    from pgrc_amd import synth
    nproc = os.cpu_count() or 1
    threads = nproc if args.cpu_threads <= 0 else max(1, min(args.cpu_threads, nproc))
    t_prep = time.perf_counter()
    pg = host_text(ctx, G)
    ns = min(args.cpu_sample_reads, n_per)
    if hasattr(ctx, "_host_rows"):
        ns = min(ns, int(ctx._host_rows[1]))       # (the sample stays inside the LQ set: the N set is the end of the sum set)
    reads = synth.reads_host(g, pg, rs, 0, ns)
    prep_s = time.perf_counter() - t_prep
    kind = "reference" if orc.have_ref() else "port"

    def run(n, thr):
        t = time.perf_counter()
        if kind == "reference":
            r = orc.ref_match("c", pg, reads[:n], seed_len, kmax, 0, True, 0, thr, thr)     # (index threads = loop threads = -t)
        else:
            r = orc.oracle_match("c", pg, reads[:n], seed_len, kmax, 0, True, thr)
        return time.perf_counter() - t, r

    def leg(thr, n_small, n_big):
        """two runs -> fixed seconds a, seconds per read b, the rate extrapolated to the workload's read count"""
        t_small, _ = run(n_small, thr)
        t_big, r = run(n_big, thr)
        b = max((t_big - t_small) / (n_big - n_small), 1e-12)
        a = max(t_small - b * n_small, 0.0)
        return {"value": n_per / (a + b * n_per), "unit": "reads/s", "cores": thr, "extrapolated": True, "fixed_s": a, "per_read_us": b * 1e6,
                "sample": f"n={n_small}: {t_small:.2f}s, n={n_big}: {t_big:.2f}s"}, r

    main, r = leg(threads, max(1000, ns // 100), ns)
    # The sample is also compared with the GPU result on the same reads.  NOTE: timed at `threads` > 1 the
    # reference builds its copMEM index with its racy multithreaded code (CopMEMMatcher.cpp:238-254, :284-305;
    # which of a crowded bucket's entries survive the 13-entry cap varies from run to run), so a small number
    # of reads in repeats legitimately differ; bit-parity is pinned against the SERIAL index build
    # (tests/fullscale_parity.py, tests/).
    pos, rc, mism, _, _ = ctx.get_results()
    diff = int((mism[:ns] != r["mism"]).sum())
    t16 = None
    if threads != min(16, nproc) and nproc >= 16:
        t16, _ = leg(16, max(1000, ns // 100), ns)
    # the same path at -t 1: serial index build, one thread in the per-read loop, on a smaller sample of the same reads
    # (two runs again: the fixed cost is two serial index builds over the whole text)
    t1 = None
    if not args.no_cpu_t1 and kind == "reference" and threads != 1:
        t1, _ = leg(1, 1000, min(50_000, ns))
        t1["sample"] += " (PgHelpers::numberOfThreads = 1, one OpenMP thread)"
    cpu_model = None
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                cpu_model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": main["value"], "unit": "reads/s", "cores": threads, "nproc": nproc, "cpu_model": cpu_model, "t16": t16, "t1": t1, "kind": kind, "extrapolated": True,
            "sample": f"EXTRAPOLATED from a bounded sample: whole {G}-bp Pg, first {ns} reads of the workload, both strands incl. index builds; two runs "
                      f"({main['sample']}) => fixed {main['fixed_s']:.2f}s + {main['per_read_us']:.3f}us/read, "
                      f"extrapolated to {n_per} reads",
            "fixed_s": main["fixed_s"], "per_read_us": main["per_read_us"], "prep_s": prep_s,
            "sample_reads_with_other_mismatch_count_than_gpu": diff,
            "note": "reference timed as shipped at -t %d (racy multithreaded index build); bit-parity is pinned against "
                    "its serial index build elsewhere" % threads}


_TEXT = {}


def host_text(ctx, G):
    """ASCII copy of the text in HBM (checker input), unpacked once"""
    if G not in _TEXT:
        _TEXT[G] = unpack_pg_to_ascii(ctx.export_pg(0))[:G]
    return _TEXT[G]


def reads_from_hbm(ctx_reads, idx, nw, stride, L):
    """the ASCII rows of reads `idx`, unpacked from the word-major 2-bit read set in HBM (exactly what the GPU matched)"""
    import numpy as np
    import torch
    ix = torch.as_tensor(idx.astype(np.int64), device=ctx_reads.device)
    rows = torch.stack([ctx_reads[w * stride + ix] for w in range(nw)], dim=1).cpu().numpy().view(np.uint32)     # (ns, nw)
    sym = (rows[:, :, None] >> (2 * np.arange(16, dtype=np.uint32))[None, None, :]) & 3
    return np.frombuffer(b"ACGT", dtype=np.uint8)[sym.reshape(idx.size, nw * 16)[:, :L]]


def rows_from_host_sets(host_rows, idx, L):
    """the ASCII rows of reads `idx` of an LQ + N sum set held in the reference's two packings (SymbolsPackingFacility:
    ACGT 4 symbols per byte, ACGNT 3 per byte as base-5 digits, first symbol most significant)"""
    import numpy as np
    lq_rows, n_lq, n_rows, n_n = host_rows
    out = np.empty((idx.size, L), dtype=np.uint8)
    is_lq = idx < n_lq
    b = lq_rows[idx[is_lq]]                                             # (k, ceil(L/4))
    sym = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=2).reshape(b.shape[0], -1)[:, :L]
    out[is_lq] = np.frombuffer(b"ACGT", dtype=np.uint8)[sym]
    c = n_rows[idx[~is_lq] - n_lq].astype(np.uint32)                    # (k, ceil(L/3))
    sym = np.stack([c // 25, (c // 5) % 5, c % 5], axis=2).reshape(c.shape[0], -1)[:, :L]
    out[~is_lq] = np.frombuffer(b"ACGNT", dtype=np.uint8)[sym]
    return out


def parity_sample(args, ctx, g, rs, n_per, L, G, seed_len, kmax):
    """Bit-parity evidence inside the bench line: a sample of the workload's reads -- a stride over ALL of them plus a
    stride over the reads the dual kernel had to do again in the reference's order (`redo_reads`: the ones in repeat
    families, where the falses budget matters) -- matched by the reference with its SERIAL canonical index build
    (PgHelpers::numberOfThreads = 1) and one thread in its per-read loop (its RC-flag race) against the whole text,
    compared with what the GPU run above produced for the same reads.  The sample's rows are read back from HBM.
    Outside the timed region; the oracle port stands in where oracle/_ref is absent."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as orc
    ns = min(args.parity_sample_reads, n_per)
    redo = np.flatnonzero(ctx.redo_flags())
    n_redo = min(redo.size, max(ns // 5, min(ns, 10_000)))
    pick_redo = redo[np.linspace(0, redo.size - 1, n_redo).astype(np.int64)] if n_redo else redo[:0]
    n_all = ns - n_redo
    pick_all = np.linspace(0, n_per - 1, n_all).astype(np.int64) if n_all > 0 else np.zeros(0, dtype=np.int64)
    idx = np.unique(np.concatenate([pick_all, pick_redo.astype(np.int64)]))
    pg = host_text(ctx, G)
    nw, stride = (L + 15) // 16, (n_per + 63) & ~63
    reads = rows_from_host_sets(ctx._host_rows, idx, L) if hasattr(ctx, "_host_rows") else reads_from_hbm(ctx._keep_reads, idx, nw, stride, L)
    # (the reads with N are the last of the set, hence of the sorted sample: the reference takes them as its N read set)
    n_nset = int((idx >= ctx._host_rows[1]).sum()) if hasattr(ctx, "_host_rows") else 0
    t = time.perf_counter()
    if orc.have_ref():
        r = orc.ref_match("c", pg, reads, seed_len, kmax, 0, True, n_nset, 1, 1)
        checker = "reference, serial index (PgHelpers::numberOfThreads = 1)"
    else:
        r = orc.oracle_match("c", pg, reads, seed_len, kmax, 0, True, max(1, min(args.cpu_threads, os.cpu_count() or 1)))
        checker = "oracle port"
    secs = time.perf_counter() - t
    pos, rc, mism, _, _ = ctx.get_results()
    d_pos = int((pos[idx] != r["pos"]).sum())
    d_rc = int((rc[idx] != r["rc"]).sum())
    d_mism = int((mism[idx] != r["mism"]).sum())
    return {"reads": int(idx.size), "drawn": f"stride over all {n_per} reads ({n_all}) + stride over the {redo.size} reads the dual kernel redid ({n_redo})",
            "redo_in_sample": int(np.isin(idx, redo).sum()), "redo_reads": int(redo.size), "reads_with_N_in_sample": n_nset,
            "checker": checker, "diff": d_pos + d_rc + d_mism, "diff_pos": d_pos, "diff_rc": d_rc,
            "diff_mism": d_mism, "matched_in_sample": int((r["mism"] != 255).sum()), "rc_in_sample": int(r["rc"].sum()), "checker_s": secs}


if __name__ == "__main__":
    main()
