"""Rate of the archive form of a reads list's mismatch streams on the device (pgrc_list_archive_encode and
pgrc_decode_add_list_archive).

100 M entries at L = 150.  No committed C3 bench line carries the mismatch histogram of its reads list, so the counts are
synthetic: 70 % zero and a geometric tail (P(c) ~ 0.55^c for c = 1 .. 12).  Each call is timed from pageable host memory,
after a warm-up, several times; device times are the library's HIP-event figures.  pgrc_decode_add_list with the streams
reassembled on the host runs beside pgrc_decode_add_list_archive in the same process; the host reassembly (numpy,
tests/listarchive_util.load_parallel's split inverse) is timed separately and is no part of the ratio.  Prints one JSON object:
per phase the median and the spread of the repeats.

    python tools/listarchive_rate.py [--entries N] [--repeats R] [--out profiles/....json]
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

import listarchive_util as la  # noqa: E402

PHASES = ("ms_flags_device", "ms_symbols_device", "ms_split_device")
COUNTS = tuple(range(1, 13))
WEIGHTS = tuple(0.55 ** c for c in COUNTS)


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def summary(runs):
    res = {k: stat(r[k] for r in runs) for k in PHASES}
    res["ms_device_total"] = stat(sum(r[k] for k in PHASES) for r in runs)
    res.update(ms_upload_host=stat(r["ms_upload"] for r in runs), ms_download_host=stat(r["ms_download"] for r in runs),
               ms_call=stat(r["ms_call"] for r in runs), ms_python_wall=stat(r["wall_python"] for r in runs),
               bytes_up=int(runs[0]["bytes_up"]), bytes_down=int(runs[0]["bytes_down"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pgrc_amd import PgRCDecoder

    n, L = args.entries, 150
    t0 = time.time()
    cnt, sym, rev_off = la.make_list(2026, n, L, zero=0.7, counts=COUNTS, weights=WEIGHTS)
    t_gen = time.time() - t0
    res = {"what": "pgrc_list_archive_encode (normal level), pgrc_decode_add_list_archive and pgrc_decode_add_list, one context each",
           "entries": n, "mismatches": int(sym.size), "L": L, "counts": "synthetic: 70 % zero, P(c) ~ 0.55^c for c = 1 .. 12",
           "repeats": args.repeats, "host_memory": "pageable"}
    dec = PgRCDecoder(L, device=0)
    runs, st = [], None
    for _ in range(args.repeats + 1):                        # (the first call sizes the buffers)
        c0 = time.perf_counter()
        st = dec.list_archive_encode(cnt, sym, rev_off)
        wall = (time.perf_counter() - c0) * 1e3
        runs.append(dict(dec.list_archive_timing(), wall_python=wall))
    res["encode"] = summary(runs[1:])
    res["limit"] = int(st["props"][0])
    res["n_nonzero"] = int(st["n_nonzero"])
    t0 = time.time()
    la.assert_streams(st, la.encode_parallel(cnt, sym, rev_off))
    res["host_encode_parallel_form_s"] = round(time.time() - t0, 1)

    dec.set_text(b"ACGT" * 64)
    runs = []
    for _ in range(args.repeats + 1):
        dec.set_text(b"ACGT" * 64)
        c0 = time.perf_counter()
        dec.add_list_archive(n, st)
        wall = (time.perf_counter() - c0) * 1e3
        runs.append(dict(dec.list_archive_timing(), wall_python=wall, ms_lists_device=dec.timing()["ms_lists_device"]))
    res["add_list_archive"] = summary(runs[1:])
    res["add_list_archive"]["ms_lists_device"] = stat(r["ms_lists_device"] for r in runs[1:])

    # the same list through pgrc_decode_add_list: the caller reassembles the streams first (timed apart)
    t0 = time.perf_counter()
    hcnt, hsym, hoff = la.load_parallel(st, L)
    res["host_reassembly_numpy_s"] = round(time.perf_counter() - t0, 2)
    assert np.array_equal(hcnt, cnt)
    plain = []
    for _ in range(args.repeats + 1):
        dec.set_text(b"ACGT" * 64)
        c0 = time.perf_counter()
        dec.add_list(n, 0, mis_cnt=hcnt, mis_sym=hsym, mis_off=hoff, mis_off_rev_coded=False, mis_sym_form=0, bases_order=st["bases_order"])
        plain.append({"wall_python": (time.perf_counter() - c0) * 1e3, "ms_lists_device": dec.timing()["ms_lists_device"]})
    res["add_list_host_reassembled"] = {"ms_python_wall": stat(r["wall_python"] for r in plain[1:]),
                                        "ms_lists_device": stat(r["ms_lists_device"] for r in plain[1:]), "bytes_up": int(n + 2 * sym.size)}
    res["ratio_add_list_archive_over_add_list_wall"] = round(res["add_list_archive"]["ms_python_wall"]["median"] /
                                                             res["add_list_host_reassembled"]["ms_python_wall"]["median"], 3)
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
