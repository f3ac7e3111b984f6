"""Rate of the pair-position coding of the order-preserving paired mode on the device (pgrc_pairpos_encode,
pgrc_decode_set_order_pair_streams) against the way to the same state that needs the finished
position array on the host: pgrc_decode_set_order with orgIdx2PgPos.

100 M reads (50 M pairs), 4-byte positions below 2^31, tests/pairpos_util's default mix of pair kinds.  One context holds
a text of 2^31 bytes and one reads list without positions (an ORD job's HQ list), so that both calls run all of
set_order's checks.  The two ways are timed in turn from pageable host memory, after a warm-up, several times; device
times are the library's HIP-event figures.  Prints one JSON object: per phase the median and the spread of the repeats.

    python tools/pairpos_rate.py [--pairs P] [--repeats R] [--out profiles/....json]
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

import pairpos_util as pp  # noqa: E402


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pgrc_amd import PgRCDecoder
    from pgrc_amd.decode import PGRC_DECODE_ORD

    P, L, W = args.pairs, 100, 4
    text_len = 1 << 31
    t0 = time.time()
    org = pp.make_positions(2024, P, W, top=text_len - L - 1, **pp.DEFAULT_MIX)
    fm = pp.file_major(org)
    t_gen = time.time() - t0

    dec = PgRCDecoder(L, device=0)
    dec.set_text(np.zeros(text_len, np.uint8))
    dec.add_list(2 * P)                                      # no positions: every row is an ORD row of this list

    enc, st = [], None
    for _ in range(args.repeats + 1):                        # (the first call sizes the buffers)
        c0 = time.perf_counter()
        st = dec.compressReadsPgPositions(org, W)
        wall = (time.perf_counter() - c0) * 1e3
        enc.append(dict(dec.pairpos_timing(), wall_python=wall))
    enc = enc[1:]
    assert np.array_equal(dec.decompressReadsPgPositions(st), fm), "the device round trip differs from the input"
    assert pp.streams_equal(st, pp.compress_states(org, W)), "the device's streams differ from the three-state form's"
    up_streams = int(sum(np.asarray(st[k]).nbytes for k in pp.STREAMS))

    new, old = [], []
    for k in range(args.repeats + 1):                        # the two ways in turn
        c0 = time.perf_counter()
        dec.set_order(PGRC_DECODE_ORD, fm.size, org_idx_to_pos=fm, paired=True, rev_compl_pair_file=True)
        wall = (time.perf_counter() - c0) * 1e3
        old.append({"wall": wall, "ms_order_device": dec.timing()["ms_order_device"]})
        c0 = time.perf_counter()
        dec.set_order_pair_streams(st, rev_compl_pair_file=True)
        wall = (time.perf_counter() - c0) * 1e3
        new.append(dict(dec.pairpos_timing(), wall=wall, ms_order_device=dec.timing()["ms_order_device"]))
    new, old = new[1:], old[1:]
    dec.close()

    dev = lambda r: r["ms_sort_device"] + r["ms_scan_device"] + r["ms_scatter_device"]  # noqa: E731
    res = {
        "what": "pair-position coding on the device against pgrc_decode_set_order with the host array, same process and context",
        "reads": 2 * P, "pairs": P, "pos_width": W, "mix": "tests/pairpos_util.DEFAULT_MIX", "mix_knobs": pp.DEFAULT_MIX,
        "kinds": pp.kinds(st), "ties": pp.ties(org), "repeats": args.repeats, "host_memory": "pageable",
        "encode": {
            "ms_sort_device": stat(r["ms_sort_device"] for r in enc), "ms_scan_device": stat(r["ms_scan_device"] for r in enc),
            "ms_scatter_device": stat(r["ms_scatter_device"] for r in enc), "ms_device_total": stat(dev(r) for r in enc),
            "ms_upload_host": stat(r["ms_upload"] for r in enc), "ms_download_host": stat(r["ms_download"] for r in enc),
            "ms_call": stat(r["ms_call"] for r in enc), "ms_python_wall": stat(r["wall_python"] for r in enc),
            "bytes_up": int(enc[0]["bytes_up"]), "bytes_down": int(enc[0]["bytes_down"]),
        },
        "set_order_pair_streams": {
            "ms_sort_device": stat(r["ms_sort_device"] for r in new), "ms_scan_device": stat(r["ms_scan_device"] for r in new),
            "ms_scatter_device": stat(r["ms_scatter_device"] for r in new), "ms_device_total": stat(dev(r) for r in new),
            "ms_order_checks_device": stat(r["ms_order_device"] for r in new), "ms_upload_host": stat(r["ms_upload"] for r in new),
            "ms_call": stat(r["ms_call"] for r in new), "ms_python_wall": stat(r["wall"] for r in new),
            "bytes_up": int(new[0]["bytes_up"]),
        },
        "set_order_host_array": {
            "ms_upload_and_checks_device": stat(r["ms_order_device"] for r in old), "ms_python_wall": stat(r["wall"] for r in old),
            "bytes_up": int(fm.nbytes),
        },
        "streams_bytes": up_streams,
        "wall_ratio_new_over_old": round(stat(r["wall"] for r in new)["median"] / stat(r["wall"] for r in old)["median"], 3),
        "host_generate_s": round(t_gen, 1),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
