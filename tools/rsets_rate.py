"""Rate of the edits of the divided read sets on the device (include/pgrc_readsets.h).

--reads reads of 150 bp split 80 / 15 / 5 % into the HQ / LQ / N set (rows of random packed bytes: the edits never look inside
a row).  A move of 20 % of the HQ set (pgrc_rsets_move_lq, the flags already on the device), then a removal of 60 % of LQ + N
(pgrc_rsets_remove).  After a warm-up the pair is repeated on a fresh object; device times by phase and the call's wall time
are the library's figures (pgrc_rsets_get_timing).  Beside them, in the same process:
  yardstick   a device-to-device hipMemcpyAsync of as many bytes as the row mover wrote, HIP events around it; the mover reads
              row bytes + 4 (its descriptor) and writes row bytes where the copy reads and writes row bytes
  host route  what a caller does without the object: flags down, rows down, a vectorised numpy compaction and merge, rows up
              again (generous to the host: the reference's loops are serial)
--reference-cpu times the reference's own four loops through the driver of tests/golden/make_golden_rsets.py on
--reference-cpu-reads reads, where oracle/_ref and the reference tree are present.  Prints one JSON object.

    python tools/rsets_rate.py [--reads R] [--repeats N] [--out profiles/rsets_rate.json] [--reference-cpu] [--skip-device]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 150
RB = (38, 38, 50)


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def generate(R, seed):
    rng = np.random.default_rng(seed)
    u = rng.random(R)
    cls = np.where(u < 0.8, 0, np.where(u < 0.95, 1, 2)).astype(np.uint8)
    cnt = [int((cls == k).sum()) for k in range(3)]
    rows = [rng.integers(0, 125 if k == 2 else 256, size=(cnt[k], RB[k]), dtype=np.uint8) for k in range(3)]
    batch = {"n_hq": cnt[0], "n_lq": cnt[1], "n_n": cnt[2], "symbols": (4, 4, 5), "row_bytes": RB, "hq_rows": rows[0], "lq_rows": rows[1],
             "n_rows": rows[2], "lq_index": np.flatnonzero(cls == 1).astype(np.uint32), "n_index": np.flatnonzero(cls == 2).astype(np.uint32)}
    is_hq = (rng.random(cnt[0]) >= 0.2).astype(np.uint8)
    moved = int((is_hq == 0).sum())
    is_mapped = (rng.random(cnt[1] + moved + cnt[2]) < 0.6).astype(np.uint8)
    return cls, batch, is_hq, is_mapped


def device_part(args):
    import torch
    from pgrc_amd import DividedReadsSets
    hip = C.CDLL(None)                      # the HIP runtime the library runs on, already loaded
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    cls, batch, is_hq, is_mapped = generate(args.reads, 1)
    d_is_hq, d_is_mapped = torch.from_numpy(is_hq).cuda(), torch.from_numpy(is_mapped).cuda()
    torch.cuda.synchronize()
    times = {"move": [], "remove": []}
    info = {}
    for rep in range(args.repeats + 1):
        s = DividedReadsSets(L, True, False)
        t0 = time.perf_counter()
        s.append(batch)
        s.finish()
        info["ms_append_from_host"] = round((time.perf_counter() - t0) * 1e3, 1)
        s.move_lq(d_is_hq.data_ptr(), on_device=True)
        tm = s.timing()
        s.remove(d_is_mapped.data_ptr(), on_device=True)
        tr = s.timing()
        if rep:                             # (the first pair is the warm-up)
            times["move"].append(tm)
            times["remove"].append(tr)
        info["counts_after"] = s.info()["count"]
        if rep < args.repeats:
            s.close()
    out = {"reads": args.reads, "read_len": L, "repeats": args.repeats, "counts": [batch["n_hq"], batch["n_lq"], batch["n_n"]],
           "moved": int((is_hq == 0).sum()), "removed": int(is_mapped.sum()), **info}
    for edit, ts in times.items():
        o = {k: stat([t[k] for t in ts]) for k in ("ms_checks_device", "ms_desc_device", "ms_rows_device", "ms_call")}
        o["rows_moved"], o["bytes_moved"] = int(ts[0]["rows_moved"]), int(ts[0]["bytes_moved"])
        # the yardstick: as many bytes, device to device
        nbytes = o["bytes_moved"]
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        src.random_(0, 256)
        ms = []
        for rep in range(args.repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.current_stream().cuda_stream
            a.record()
            if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream):      # hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")
            b.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(a.elapsed_time(b))
        o["ms_memcpy_d2d"] = stat(ms)
        o["rows_over_memcpy"] = round(o["ms_rows_device"]["median"] / o["ms_memcpy_d2d"]["median"], 3)
        o["rows_GBps_written"] = round(nbytes / o["ms_rows_device"]["median"] / 1e6, 1)
        del src, dst
        out[edit] = o
    # the host route for the move: flags down, HQ and LQ rows down, numpy, both sets up again
    host = {k: [] for k in ("ms_flags_down", "ms_rows_down", "ms_numpy", "ms_rows_up", "ms_total")}
    s2 = DividedReadsSets(L, True, False)
    s2.append(batch)
    s2.finish()
    for rep in range(min(args.repeats, 3) + 1):
        t0 = time.perf_counter()
        f = d_is_hq.cpu().numpy().astype(bool)
        t1 = time.perf_counter()
        hq, lq = s2.get_rows("hq"), s2.get_rows("lq")
        t2 = time.perf_counter()
        c = cls.copy()
        hq_idx = np.flatnonzero(c == 0)
        c[hq_idx[~f]] = 3
        to_lq = np.flatnonzero((c == 1) | (c == 3))
        new_lq = np.empty((to_lq.size, RB[1]), np.uint8)
        from_lq = c[to_lq] == 1
        new_lq[from_lq] = lq
        new_lq[~from_lq] = hq[~f]
        new_hq = hq[f]
        new_map = np.concatenate([to_lq, [args.reads]]).astype(np.uint32)
        t3 = time.perf_counter()
        up = [torch.from_numpy(new_hq).cuda(), torch.from_numpy(new_lq).cuda(), torch.from_numpy(new_map).cuda()]
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        del up
        if rep:
            for k, v in zip(host, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                host[k].append(v * 1e3)
    out["host_route_move"] = {k: stat(v) for k, v in host.items()}
    out["host_route_over_device_call"] = round(out["host_route_move"]["ms_total"]["median"] / out["move"]["ms_call"]["median"], 1)
    s2.close()
    return out


def reference_cpu(n):
    """the reference's own loops on n reads: ms of the four member functions"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden_rsets as mg
    rng = np.random.default_rng(3)
    u = rng.random(n)
    plan = np.where(u < 0.64, mg.HQ, np.where(u < 0.8, mg.MOVED, np.where(u < 0.95, mg.LQ, mg.N))).astype(np.uint8)
    reads, quals = mg.records(rng, plan, L, True)
    in_hq = (plan == mg.HQ) | (plan == mg.MOVED)
    is_hq = (plan[in_hq] == mg.HQ).astype(np.uint8)
    is_mapped = (rng.random(int((plan != mg.HQ).sum())) < 0.6).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        exe = mg.build_driver(tmp)
        for fname, a in (("reads", reads), ("quals", quals), ("is_hq", is_hq), ("is_mapped", is_mapped)):
            a.tofile(os.path.join(tmp, fname))
        r = subprocess.run([exe, tmp, str(L), "1", str(mg.ERROR_LIMIT), "time"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    ms = [float(x) for x in r.stderr.strip().split("\n")[-1].split()[1:]]
    return {"reads": n, "ms_move": ms[0], "ms_hq_mapping": ms[1], "ms_remove_lq": ms[2], "ms_remove_n": ms[3], "threads": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rsets_rate.json"))
    ap.add_argument("--reference-cpu", action="store_true")
    ap.add_argument("--reference-cpu-reads", type=int, default=2_000_000)
    ap.add_argument("--skip-device", action="store_true")
    args = ap.parse_args()
    out = {}
    if not args.skip_device:
        out.update(device_part(args))
    if args.reference_cpu:
        out["reference_cpu"] = reference_cpu(args.reference_cpu_reads)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
