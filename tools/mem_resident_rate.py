"""Stage 7 (SimplePgMatcher::matchPgsInPg's matching) from texts that are already on the device, against the host route
(DESIGN.md section 4.21).

The inputs of tools/pgmap_rate.py at C3 size: a synthetic 1.875 Gbp HQ with planted reverse-complement copies, a 60 Mbp LQ of HQ
stretches on both strands, and a small N text.  All three are put into HBM as ASCII first -- where pgrc_asm_run leaves an
assembled pseudogenome (pgrc_asm_text_device) -- and then, in one process, matched twice:
  host route      what a caller had to do before: the text down (get_text: a device-to-host copy of the ASCII), the reverse
                  complement on the host (numpy's table look-up; the reference's loop is serial), pgrc_mem_set_src_ascii,
                  pgrc_mem_match_texts per text
  resident route  pgrc_mem_set_src_device, pgrc_mem_match_texts_device per text
each phase timed on the host clock around the call, --repeats times after a warm-up; the matches of both routes must be equal.
Beside them the packing kernel alone (k_mem_pack_dev, mempack.hip; HIP events through libpgrc_selftest.so), forward and
reversed, at the HQ's and the LQ's size, and a device-to-device hipMemcpyAsync of as many bytes as the kernel reads (it writes
3/8 of that; the copy writes all of it).  Prints one JSON object.

    python tools/mem_resident_rate.py [--pg-len G] [--lq-len N] [--n-len N] [--repeats R] [--out profiles/mem_resident_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pgmap_util as pu  # noqa: E402
from restore_rate import plant  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pg-len", type=int, default=1_875_000_000)
    ap.add_argument("--lq-len", type=int, default=60_000_000)
    ap.add_argument("--n-len", type=int, default=2_000_000)
    ap.add_argument("--target-len", type=int, default=45)
    ap.add_argument("--copies", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mem_resident_rate.json"))
    args = ap.parse_args()
    import torch
    import memdev_util as mu
    from pgrc_amd import CopMEMMatcher, synth

    G, GL, GN, tl = args.pg_len, args.lq_len, args.n_len, args.target_len
    t0 = time.time()
    hq = synth.pg_host(synth.pg_params(G, seed=77, tandem_every=64))
    rng = np.random.default_rng(77)
    plant(hq, rng, args.copies, 3)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    lq = rng.choice(acgt, size=GL)
    for _ in range(GL // 3000):
        ln = int(rng.integers(100, 2000))
        s, d = int(rng.integers(0, G - ln)), int(rng.integers(0, GL - ln))
        lq[d:d + ln] = pu.revcomp_np(hq[s:s + ln]) if rng.random() < 0.7 else hq[s:s + ln]
    nt = rng.choice(acgt, size=GN)
    for _ in range(GN // 3000):
        ln = int(rng.integers(100, 600))
        s, d = int(rng.integers(0, G - ln)), int(rng.integers(0, GN - ln))
        nt[d:d + ln] = pu.revcomp_np(hq[s:s + ln])
    nt[rng.integers(0, GN, size=GN // 150)] = ord("N")
    t_gen = time.time() - t0
    texts = {"hq": hq, "lq": lq, "n": nt}
    d_text = {k: torch.from_numpy(v).cuda() for k, v in texts.items()}      # where the assembler leaves them
    torch.cuda.synchronize()
    order = (("lq", False), ("n", False), ("hq", True))                     # matchPgsInPg's calls: the HQ against itself last

    host = {k: [] for k in ("ms_get_text", "ms_host_revcomp", "ms_set_src_ascii", "ms_match_texts", "ms_total")}
    res = {k: [] for k in ("ms_set_src_device", "ms_match_texts_device", "ms_total")}
    per_text = {"host": {k: [] for k in texts}, "resident": {k: [] for k in texts}}
    found = {}
    down = {k: np.empty(v.size, dtype=np.uint8) for k, v in texts.items()}
    down_t = {k: torch.from_numpy(v) for k, v in down.items()}             # (pageable host memory, as a caller's std::string is)

    def get_texts():
        for k in texts:
            down_t[k].copy_(d_text[k])
        torch.cuda.synchronize()

    for rep in range(args.repeats + 1):
        # ---- host route
        _, ms_get = clock(get_texts)
        rc, ms_rc = clock(lambda: {k: pu.revcomp_np(down[k]) for k in texts})
        tm, ms_src = clock(lambda: CopMEMMatcher(down["hq"], tl, device=0))
        ms_match = 0.0
        for name, dis in order:
            f, ms = clock(lambda: tm.matchTexts(rc[name], dis, True))
            ms_match += ms
            if rep:
                per_text["host"][name].append(ms)
            found[("host", name)] = f
        tm.close()
        del rc
        if rep:
            for k, v in zip(host, (ms_get, ms_rc, ms_src, ms_match, ms_get + ms_rc + ms_src + ms_match)):
                host[k].append(v)
        # ---- resident route
        tm = CopMEMMatcher(None, tl, device=0)
        _, ms_src = clock(lambda: tm.setSrcDevice(d_text["hq"].data_ptr(), G))
        ms_match = 0.0
        for name, dis in order:
            f, ms = clock(lambda: tm.matchTextsDevice(d_text[name].data_ptr(), texts[name].size, dis, True))
            ms_match += ms
            if rep:
                per_text["resident"][name].append(ms)
            found[("resident", name)] = f
        tm.close()
        if rep:
            for k, v in zip(res, (ms_src, ms_match, ms_src + ms_match)):
                res[k].append(v)
    equal = all(np.array_equal(found[("host", k)], found[("resident", k)]) for k in texts)

    # ---- the packing kernel beside a device-to-device copy of the bytes it reads
    lib = mu.lib()
    lib.pgrc_selftest_mem_pack_time.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(C.c_float)]
    hip = C.CDLL(None)                      # the HIP runtime the library runs on, already loaded
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    st = mu.MemPack(0)
    kernel = {}
    reps = max(args.repeats, 3) + 1
    for name in ("hq", "lq"):
        n = texts[name].size
        o = {"bytes_read": n, "bytes_written": ((n + 15) // 16 + mu.PAD_WORDS) * 6}
        for label, rev, off, cut in (("forward", 0, 0, 0), ("reversed", 1, 0, 0), ("reversed_unaligned", 1, 5, 6)):     # (start, end) bytes cut off
            ms = (C.c_float * reps)()
            st._check(lib.pgrc_selftest_mem_pack_time(st.h, C.c_void_p(d_text[name].data_ptr() + off), n - off - cut, rev, reps, ms), "mem_pack_time")
            o["ms_" + label] = spread(list(ms)[1:])
        dst = torch.empty(n, dtype=torch.uint8, device="cuda")
        ms = []
        for rep in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if hip.hipMemcpyAsync(dst.data_ptr(), d_text[name].data_ptr(), n, 3, torch.cuda.current_stream().cuda_stream):    # hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")
            b.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(a.elapsed_time(b))
        del dst
        o["ms_memcpy_d2d"] = spread(ms)
        o["reversed_over_memcpy"] = round(o["ms_reversed"]["median"] / o["ms_memcpy_d2d"]["median"], 3)
        o["reversed_GBps_read"] = round(n / o["ms_reversed"]["median"] / 1e6, 1)
        kernel[name] = o
    st.close()

    out = {
        "what": "stage 7's matching from device-resident ASCII texts (pgrc_mem_set_src_device / pgrc_mem_match_texts_device) beside the host route, one process",
        "pg_len": G, "lq_len": GL, "n_len": GN, "target_len": tl, "repeats": args.repeats,
        "matches": {k: int(found[("resident", k)].shape[0]) for k in texts}, "routes_equal": bool(equal),
        "host_route": {k: spread(v) for k, v in host.items()},
        "resident_route": {k: spread(v) for k, v in res.items()},
        "match_call_ms": {r: {k: spread(v) for k, v in d.items()} for r, d in per_text.items()},
        "host_over_resident": round(statistics.median(host["ms_total"]) / statistics.median(res["ms_total"]), 2),
        "ms_saved": round(statistics.median(host["ms_total"]) - statistics.median(res["ms_total"]), 1),
        "packing_kernel": kernel,
        "host_generate_s": round(t_gen, 1),
    }
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
