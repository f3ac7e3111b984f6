"""Rate of the pair-order coding of the paired mode that does not preserve the order on the device (pgrc_pairorder_encode;
DESIGN.md section 4.11).

100 M entries (50 M pairs) in the FILE_FLAGS form, which PgRC uses by default on paired input, from two orders: the
generator's default mix (tests/pairorder_util.make_order: most mates lie near their base, as in orders that come from a
pseudogenome) and a uniformly random permutation, the worst case for the scatter of rev and the gather of the mates (one
128-byte line per entry).  Each is timed from pageable host memory, after a warm-up, several times; device times are the
library's HIP-event figures.  Prints one JSON object: per phase the median and the spread of the repeats.

    python tools/pairorder_rate.py [--pairs P] [--repeats R] [--out profiles/....json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pairorder_util as po  # noqa: E402

PHASES = ("ms_inverse_device", "ms_scatter_device", "ms_scan_device", "ms_compact_device")


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def measure(dec, org, form, repeats):
    runs, st = [], None
    for _ in range(repeats + 1):                             # (the first call sizes the buffers)
        c0 = time.perf_counter()
        st = dec.compressReadsOrder(org, form)
        wall = (time.perf_counter() - c0) * 1e3
        runs.append(dict(dec.pairorder_timing(), wall_python=wall))
    runs = runs[1:]
    assert po.streams_equal(st, po.compress_parallel(org, form)), "the device's streams differ from the parallel form's"
    res = {k: stat(r[k] for r in runs) for k in PHASES}
    res["ms_device_total"] = stat(r["ms_inverse_device"] + r["ms_scan_device"] + r["ms_compact_device"] for r in runs)
    res.update(ms_upload_host=stat(r["ms_upload"] for r in runs), ms_download_host=stat(r["ms_download"] for r in runs),
               ms_call=stat(r["ms_call"] for r in runs), ms_python_wall=stat(r["wall_python"] for r in runs),
               bytes_up=int(runs[0]["bytes_up"]), bytes_down=int(runs[0]["bytes_down"]), kinds=po.kinds(st))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pgrc_amd import PgRCDecoder

    P = args.pairs
    t0 = time.time()
    orders = {"default_mix": po.make_order(2024, P, **po.DEFAULT_MIX),
              "random_permutation": np.random.default_rng(2025).permutation(2 * P).astype(np.uint32)}
    t_gen = time.time() - t0
    dec = PgRCDecoder(100, device=0)
    res = {"what": "pgrc_pairorder_encode, FILE_FLAGS form, one context, orders in turn", "entries": 2 * P, "pairs": P,
           "mix_knobs": po.DEFAULT_MIX, "repeats": args.repeats, "host_memory": "pageable"}
    for name, org in orders.items():
        res[name] = measure(dec, org, po.FILE_FLAGS, args.repeats)
    dec.close()
    res["host_generate_s"] = round(t_gen, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
