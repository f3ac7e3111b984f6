"""Rate of the overlap search on the device (pgrc_ovl_run).

A generated set of --reads reads of 150 bp over ACGT from a random genome at coverage 30 with 1 % substitutions, stop
coefficient 1 (149 sweeps).  The whole call is timed after a warm-up, with the order made on the device; device times are
the library's HIP-event figures by phase and by sweep, and pgrc_ovl_assemble is timed behind it.  No time is a pass
condition; the result is checked for what any run must give (every link's overlap is real, no read has two predecessors, the
reads-left numbers fall by the links made).  Prints one JSON object.

    python tools/pgovl_rate.py [--reads R] [--repeats N] [--out profiles/pgovl_rate.json]
    python tools/pgovl_rate.py --rule parallel [--reads R] [--repeats N] [--out profiles/pgovl_rate_parallel.json]
        the rule of the parallel generator and, beside it in the same process on the same set, the
        serial rule: "parallel" and "serial" in one JSON object, each by phase and by sweep, with the rule info
    python tools/pgovl_rate.py --reference-cpu [--reads R] --out FILE     # no GPU: times the reference's serial
        findOverlappingReads on the same set with the fixture driver (needs oracle/_ref and the reference tree) and adds
        "reference_cpu" to FILE
"""
import argparse
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

L = 150
PHASES = ("ms_order_device", "ms_start_device", "ms_merge_device", "ms_pair_device", "ms_compact_device")


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def generate(R, seed):
    """-> codes uint8 [R, L]"""
    rng = np.random.default_rng(seed)
    glen = max(L + 1, R * L // 30)
    genome = rng.integers(0, 4, size=glen, dtype=np.uint8)
    codes = np.empty((R, L), dtype=np.uint8)
    for at in range(0, R, 1 << 20):
        n = min(R, at + (1 << 20)) - at
        pos = rng.integers(0, glen - L + 1, size=n)
        c = genome[pos[:, None] + np.arange(L)[None, :]]
        err = rng.random(c.shape) < 0.01
        c[err] = (c[err] + rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)) & 3
        codes[at:at + n] = c
    return codes


def pack(codes):
    R = codes.shape[0]
    pad = np.zeros((R, (L + 3) // 4 * 4), dtype=np.uint8)
    pad[:, :L] = codes
    return (pad.reshape(R, -1, 4) * np.array([64, 16, 4, 1], dtype=np.uint8)).sum(axis=2, dtype=np.uint8)


def check(codes, out):
    nx, ov = out["next_read"].astype(np.int64), out["overlap"].astype(np.int64)
    R = codes.shape[0]
    src = np.flatnonzero(nx[1:]) + 1
    assert np.unique(nx[src]).size == src.size, "a read with two predecessors"
    assert src.size == out["duplicates"] + out["links"] and int(out["reads_left"][-1]) == R - src.size
    for at in range(0, src.size, 1 << 18):                  # every link's overlap is real
        s = src[at:at + (1 << 18)]
        o = ov[s]
        k = np.arange(L)[None, :]
        a = codes[s - 1][np.arange(s.size)[:, None], np.minimum(L - o[:, None] + k, L - 1)]
        b = codes[nx[s] - 1]
        assert ((a == b) | (k >= o[:, None])).all(), "a link whose overlap is not real"


def reference_cpu(args):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_pgovl", os.path.join(ROOT, "tests", "golden", "make_golden_pgovl.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    codes = generate(args.reads, 2026)
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    with tempfile.TemporaryDirectory() as tmp:
        ms = mk.reference_ms(mk.build_driver(tmp), tmp, reads, L, 4, 1.0)
    res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    cpu = "unknown"
    for ln in open("/proc/cpuinfo"):
        if ln.startswith("model name"):
            cpu = ln.split(":", 1)[1].strip()
            break
    res["reference_cpu"] = {"what": "the reference's findOverlappingReads at one thread (initAndFindDuplicates and the sweeps), same generated set", "reads": args.reads,
                            "ms": round(ms, 1), "machine": f"{cpu}, {os.cpu_count()} logical CPUs, {platform.system()} {platform.machine()}"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference-cpu", action="store_true")
    ap.add_argument("--rule", choices=("serial", "parallel"), default="serial")
    args = ap.parse_args()
    if args.reference_cpu:
        return reference_cpu(args)
    from pgrc_amd import OverlapFinder, PgAssembler

    R = args.reads
    t0 = time.time()
    codes = generate(R, 2026)
    rows = pack(codes)
    t_gen = time.time() - t0
    print(f"generated {R} reads in {t_gen:.1f} s", file=sys.stderr, flush=True)
    ovl, asm = OverlapFinder(device=0), PgAssembler(device=0)
    res = {"what": "pgrc_ovl_run, 150 bp over ACGT from a genome at coverage 30 with 1 % substitutions, stop coefficient 1, the order made on the device; "
                   "pgrc_ovl_assemble behind it", "reads": R, "read_len": L, "repeats": args.repeats}
    if args.rule == "parallel":
        res["what"] += "; under the rule of the parallel generator and, beside it, under the serial rule"
        for rule in ("serial", "parallel"):
            res[rule] = measure(ovl, asm, rows, codes, args.repeats, rule)
            res[rule]["rule_info"] = ovl.rule_info()
    else:
        res.update(measure(ovl, asm, rows, codes, args.repeats, None))
    ovl.close()
    asm.close()
    res["host_generate_s"] = round(t_gen, 1)
    if args.rule == "serial" and args.out and os.path.exists(args.out):     # (a reference time taken earlier stays)
        old = json.load(open(args.out))
        if "reference_cpu" in old:
            res["reference_cpu"] = old["reference_cpu"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


def measure(ovl, asm, rows, codes, repeats, rule):
    """repeats timed runs behind a warm-up under `rule` (None: as the context is) -> the figures of one rule"""
    res = {}
    runs = []
    for _ in range(repeats + 1):                                # (the first call sizes the buffers)
        c0 = time.perf_counter()
        out = ovl.run(rows, L, 4, 1.0, None, rule=rule)
        c1 = time.perf_counter()
        pg = ovl.assemble(asm)
        c2 = time.perf_counter()
        runs.append(dict(ovl.timing(), wall_run=(c1 - c0) * 1e3, wall_assemble=(c2 - c1) * 1e3, asm=asm.timing()))
        print(f"run {len(runs)}: {runs[-1]['wall_run']:.0f} ms, assemble {runs[-1]['wall_assemble']:.0f} ms", file=sys.stderr, flush=True)
    first, runs = runs[0], runs[1:]
    check(codes, out)
    res.update(duplicates=int(out["duplicates"]), links=int(out["links"]), sweeps=int(out["sweeps"]), passes=int(runs[0]["passes"]),
               reads_left={str(i): int(out["reads_left"][i]) for i in (0, 1, 2, 5, 10, 20, 50, 100, 149) if i < out["reads_left"].size},
               pg_len=int(pg["pg_len"]), cycles=int(pg["cycles"]))
    r = {k: stat(x[k] for x in runs) for k in PHASES}
    r["ms_device_total"] = stat(sum(x[k] for k in PHASES) for x in runs)
    r.update(ms_upload_host=stat(x["ms_upload"] for x in runs), ms_download_host=stat(x["ms_download"] for x in runs), ms_call=stat(x["ms_call"] for x in runs),
             ms_python_run=stat(x["wall_run"] for x in runs), ms_first_call=round(first["ms_call"], 3),
             ms_assemble_call=stat(x["asm"]["ms_call"] for x in runs), ms_python_assemble=stat(x["wall_assemble"] for x in runs),
             bytes_up=int(runs[0]["bytes_up"]), bytes_down=int(runs[0]["bytes_down"]),
             ms_sweeps_device=[round(x, 3) for x in runs[-1]["ms_sweeps_device"]])
    res["device"] = r
    return res


if __name__ == "__main__":
    sys.exit(main())
