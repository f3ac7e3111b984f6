"""Rate of the pair-order coding of the paired mode that does not preserve the order on the device (pgrc_pairorder_encode;
DESIGN.md section 4.11).

100 M entries (50 M pairs) in the FILE_FLAGS form, which PgRC uses by default on paired input, from two orders: the
generator's default mix (tests/pairorder_util.make_order: most mates lie near their base, as in orders that come from a
pseudogenome) and a uniformly random permutation, the worst case for the scatter of rev and the gather of the mates (one
128-byte line per entry).  Each is timed from pageable host memory, after a warm-up, several times; device times are the
library's HIP-event figures.  Prints one JSON object: per phase the median and the spread of the repeats.

    python tools/pairorder_rate.py [--pairs P] [--repeats R] [--out profiles/....json]

--decode measures the other direction (pgrc_pairorder_decode and pgrc_decode_set_order_pair_order_streams) on the streams the
device's encoder makes of the same two orders: device time by phase (chain, landing, tail, check), the upload, both whole
calls and the landing's rounds per word -- and beside them, in the same run, what they replace: the serial loop of
decompressReadsOrder restated in plain C (below; gcc -O2, one thread) and pgrc_decode_set_order with the loop's host array.

    python tools/pairorder_rate.py --decode [--pairs P] [--repeats R] [--out profiles/pairorder_decode_rate.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
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


DECODE_PHASES = ("ms_chain_device", "ms_landing_device", "ms_tail_device", "ms_check_device")

# decompressReadsOrder (SeparatedPseudoGenomePersistence.cpp:393-440) for the FILE_FLAGS form: the serial loop and the swaps
SERIAL_C = r"""
#include <stdint.h>
#include <stdlib.h>
int serial_decode(uint64_t T, const uint8_t *f8, const uint8_t *oval, const uint8_t *dfl, const int8_t *dval, const uint32_t *full,
                  const uint8_t *off_ff, const uint8_t *nonoff_ff, uint32_t *order) {
    uint8_t *done = calloc(T ? T : 1, 1);
    if (!done) return 1;
    int64_t pair_offset = 0, pair_counter = -1, off_idx = -1, del_flag_idx = -1, del_idx = -1, ful_idx = -1, ref_prev = 0, prev = 0;
    int match = 0;
    for (uint64_t i = 0; i < T; i++) {
        if (done[i]) continue;
        if (f8[++pair_counter]) pair_offset = oval[++off_idx];
        else if (dfl[++del_flag_idx]) {
            pair_offset = ref_prev + dval[++del_idx];
            ref_prev = pair_offset;
            match = 1;
            prev = pair_offset;
        } else {
            pair_offset = full[++ful_idx];
            if (!match || ref_prev != prev) ref_prev = pair_offset;
            match = 0;
            prev = pair_offset;
        }
        order[pair_counter * 2] = (uint32_t)i;
        order[pair_counter * 2 + 1] = (uint32_t)(i + pair_offset);
        done[i + pair_offset] = 1;
    }
    int64_t a = -1, b = -1;
    for (uint64_t p = 0; p < T / 2; p++) {
        if (f8[p] ? off_ff[++a] : nonoff_ff[++b]) {
            uint32_t t = order[p * 2];
            order[p * 2] = order[p * 2 + 1];
            order[p * 2 + 1] = t;
        }
    }
    free(done);
    return 0;
}
"""


def serial_loop(tmp):
    src, so = os.path.join(tmp, "serial.c"), os.path.join(tmp, "libserial.so")
    with open(src, "w") as f:
        f.write(SERIAL_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", src, "-o", so], check=True)
    fn = ctypes.CDLL(so).serial_decode
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint64] + [ctypes.c_void_p] * 8
    return fn


def measure_decode(dec, job, serial, st, repeats):
    """job: a decoder with a text and one list of n_total entries (for the two set_order routes)"""
    T = int(st["n_total"])
    keys = ("off8_flag", "off_value", "delta8_flag", "delta_value", "full_offset", "off_base_file_flag", "nonoff_base_file_flag")
    arrs = [np.ascontiguousarray(st[k]) for k in keys]
    host = np.empty(T, np.uint32)
    runs, out = [], None
    for _ in range(repeats + 1):                             # (the first call sizes the buffers)
        c0 = time.perf_counter()
        out = dec.decompressReadsOrder(st)
        wall = (time.perf_counter() - c0) * 1e3
        r = dict(dec.pairorder_decode_timing(), wall_python=wall)
        c0 = time.perf_counter()
        job.set_order_pair_order_streams(st, False)
        r["wall_set_order_streams"] = (time.perf_counter() - c0) * 1e3
        r["ms_call_set_order_streams"] = job.pairorder_decode_timing()["ms_call"]
        c0 = time.perf_counter()
        assert serial(T, *[a.ctypes.data for a in arrs], host.ctypes.data) == 0
        r["ms_serial_loop"] = (time.perf_counter() - c0) * 1e3
        c0 = time.perf_counter()
        job.set_order(1, T, rl_idx_order=host)
        r["ms_set_order_host_array"] = (time.perf_counter() - c0) * 1e3
        runs.append(r)
    runs = runs[1:]
    assert np.array_equal(out, host), "the device's order differs from the serial loop's"
    res = {k: stat(r[k] for r in runs) for k in DECODE_PHASES}
    res["ms_device_total"] = stat(sum(r[k] for k in DECODE_PHASES) for r in runs)
    res.update(ms_upload_host=stat(r["ms_upload"] for r in runs), ms_download_host=stat(r["ms_download"] for r in runs),
               ms_call_decode=stat(r["ms_call"] for r in runs), ms_python_wall_decode=stat(r["wall_python"] for r in runs),
               ms_call_set_order_streams=stat(r["ms_call_set_order_streams"] for r in runs),
               ms_python_wall_set_order_streams=stat(r["wall_set_order_streams"] for r in runs),
               ms_serial_loop_gcc_O2=stat(r["ms_serial_loop"] for r in runs),
               ms_set_order_host_array=stat(r["ms_set_order_host_array"] for r in runs),
               ms_serial_loop_plus_set_order=stat(r["ms_serial_loop"] + r["ms_set_order_host_array"] for r in runs),
               bytes_up=int(runs[0]["bytes_up"]), bytes_down=int(runs[0]["bytes_down"]), landing_words=int(runs[0]["landing_words"]),
               landing_rounds=int(runs[0]["landing_rounds"]),
               rounds_per_word=round(runs[0]["landing_rounds"] / max(1, runs[0]["landing_words"]), 3), kinds=po.kinds(st))
    return res


def main_decode(args):
    from pgrc_amd import PgRCDecoder

    P = args.pairs
    t0 = time.time()
    orders = {"default_mix": po.make_order(2024, P, **po.DEFAULT_MIX),
              "random_permutation": np.random.default_rng(2025).permutation(2 * P).astype(np.uint32)}
    t_gen = time.time() - t0
    dec = PgRCDecoder(100, device=0)
    job = PgRCDecoder(100, device=0)                        # every entry reads the one window of a text of one read
    job.set_text(np.full(100, ord("A"), np.uint8))
    job.add_list(2 * P, 0, off=np.zeros(2 * P, np.uint8))
    res = {"what": "pgrc_pairorder_decode and pgrc_decode_set_order_pair_order_streams, FILE_FLAGS form, against the serial loop in C "
                   "(gcc -O2, one thread) and pgrc_decode_set_order with its host array; medians of the repeats after a warm-up, one process",
           "entries": 2 * P, "pairs": P, "mix_knobs": po.DEFAULT_MIX, "repeats": args.repeats, "host_memory": "pageable"}
    with tempfile.TemporaryDirectory() as tmp:
        serial = serial_loop(tmp)
        for name, org in orders.items():
            st = dec.compressReadsOrder(org, po.FILE_FLAGS)
            res[name] = measure_decode(dec, job, serial, st, args.repeats)
    dec.close()
    job.close()
    res["host_generate_s"] = round(t_gen, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.decode:
        return main_decode(args)
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
