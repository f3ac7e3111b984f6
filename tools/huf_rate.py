"""Rate of the Huffman coder on the device, one process, two inputs:

  varlen   a var-len DNA coded text: the synthetic pseudogenome of pgrc_amd.synth pushed through the var-len coder with the
           encoder's book (id 0, from a recorded stream under tests/golden), cut to --coded-mib MiB (default 1 GiB)
  flags    --flags entries (default 100 M) of a rev_comp-like stream: bytes 0 and 1, evenly

Per input: a device-to-device copy of the same bytes (torch, device events); encode and decode device to device with the
coder's device time by phase; encode and decode as whole calls from and into page-locked host memory (host clock, with the
upload and download the call reports); the coded ratio; the round trip's equality; and the reference's HUF_compress2 /
HUF_decompress over the same chunks on one host core, from oracle/_ref in the same process (one pass each).  Whole calls and
phases are medians of five repeats after a warm-up, with minimum and maximum.  Prints one JSON line.

    python tools/huf_rate.py [--coded-mib 1024] [--flags 100000000] [--out profiles/huf_rate.json]
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

import huf_util as hu  # noqa: E402
import varlen_util as vu  # noqa: E402

REPEATS = 5
PHASES = ("ms_upload", "ms_tables", "ms_emit", "ms_compact", "ms_download", "ms_call")
ORDER = 17


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def timed(fn, coder=None):
    """a warm-up, then REPEATS calls -> (the last result, the calls' ms, the coder's phases per call)"""
    res = fn()
    ms, phases = [], []
    for _ in range(REPEATS):
        c0 = time.perf_counter()
        res = fn()
        ms.append((time.perf_counter() - c0) * 1e3)
        if coder is not None:
            phases.append(coder.timing())
    return res, ms, phases


def phase_spread(phases):
    return {k: spread([float(p[k]) for p in phases]) for k in PHASES}


def gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 2)


def reference_one_core(x: np.ndarray):
    """HUF_compress2 and HUF_decompress chunk by chunk on this core -> (coded bytes, compress s, decompress s); a chunk the
    reference refuses counts raw"""
    lib = hu.ref_lib()
    if lib is None:
        return None
    cap = (1 << ORDER) + 1024
    dst, back = C.create_string_buffer(cap), C.create_string_buffer(1 << ORDER)
    coded, t_c, t_d = 0, 0.0, 0.0
    for at in range(0, x.size, 1 << ORDER):
        c = x[at:at + (1 << ORDER)]
        t0 = time.perf_counter()
        r = lib.HUF_compress2(dst, cap, c.ctypes.data, c.size, 255, 11)
        t_c += time.perf_counter() - t0
        if r <= 1 or r >= c.size:
            coded += 1 if r == 1 else c.size
            continue
        coded += r
        t0 = time.perf_counter()
        got = lib.HUF_decompress(back, c.size, dst, r)
        t_d += time.perf_counter() - t0
        assert got == c.size
    return coded, t_c, t_d


def unpack_words(torch, words, n):
    """the synthetic pseudogenome as pgrc_synth_pg_device leaves it (symbol i in bits 2 (i % 16) of word i / 16) -> n ASCII symbols"""
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=words.device)
    shifts = torch.arange(16, dtype=torch.int32, device=words.device) * 2
    text = torch.empty(words.numel() * 16, dtype=torch.uint8, device=words.device)
    step = 1 << 22
    for a in range(0, words.numel(), step):
        w = words[a:a + step]
        text[a * 16:(a + w.numel()) * 16] = lut[((w[:, None] >> shifts) & 3).long()].reshape(-1)
    return text[:n]


def measure(torch, coder, d_src):
    n = int(d_src.numel())
    out = {"bytes": n}
    # the yardstick: a device-to-device copy of the same bytes
    d_copy = torch.empty_like(d_src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copies = []
    for k in range(REPEATS + 1):
        ev[0].record()
        d_copy.copy_(d_src)
        ev[1].record()
        torch.cuda.synchronize()
        if k:
            copies.append(ev[0].elapsed_time(ev[1]))
    del d_copy
    out["device_copy_ms"] = spread(copies)
    d_out = torch.empty(coder.bound(n), dtype=torch.uint8, device="cuda")
    d_coded, ms, ph = timed(lambda: coder.encode(d_src, out=d_out), coder)
    m = int(d_coded.numel())
    t = ph[-1]
    out.update(coded_bytes=m, coded_ratio=round(m / n, 4), chunks={k: int(t[k]) for k in ("chunks", "huf_chunks", "rle_chunks", "raw_chunks")})
    dev_ms = statistics.median([p["ms_tables"] + p["ms_emit"] + p["ms_compact"] for p in ph])
    out["encode_device_to_device"] = {"call_ms": spread(ms), "phases_ms": phase_spread(ph), "device_ms": round(dev_ms, 3),
                                      "GBps_of_source_device": gbps(n, dev_ms), "GBps_of_source_call": gbps(n, statistics.median(ms))}
    d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
    back, ms, ph = timed(lambda: coder.decode(d_coded, n, out=d_back), coder)
    dev_ms = statistics.median([p["ms_tables"] + p["ms_emit"] for p in ph])
    out["decode_device_to_device"] = {"call_ms": spread(ms), "phases_ms": phase_spread(ph), "device_ms": round(dev_ms, 3),
                                      "GBps_of_output_device": gbps(n, dev_ms), "GBps_of_output_call": gbps(n, statistics.median(ms))}
    out["round_trip_equal"] = bool(torch.equal(back, d_src))
    # whole calls from and into page-locked memory
    h_src = torch.empty(n, dtype=torch.uint8).pin_memory()
    h_src.copy_(d_src)
    h_coded = torch.empty(coder.bound(n), dtype=torch.uint8).pin_memory().numpy()
    h_back = torch.empty(n, dtype=torch.uint8).pin_memory().numpy()
    coded, ms, ph = timed(lambda: coder.encode(h_src.numpy(), out=h_coded), coder)
    out["encode_pinned_host"] = {"call_ms": spread(ms), "phases_ms": phase_spread(ph), "GBps_of_source_call": gbps(n, statistics.median(ms))}
    got, ms, ph = timed(lambda: coder.decode(coded, n, out=h_back), coder)
    out["decode_pinned_host"] = {"call_ms": spread(ms), "phases_ms": phase_spread(ph), "GBps_of_output_call": gbps(n, statistics.median(ms))}
    out["round_trip_equal"] = out["round_trip_equal"] and got.tobytes() == h_src.numpy().tobytes() and coded.size == m
    ref = reference_one_core(h_src.numpy())
    if ref is not None:
        out["reference_one_host_core"] = {"coded_bytes": ref[0], "coded_ratio": round(ref[0] / n, 4), "compress_s": round(ref[1], 3),
                                          "decompress_s": round(ref[2], 3), "compress_GBps": round(n / ref[1] / 1e9, 3),
                                          "decompress_GBps": round(n / ref[2] / 1e9, 3) if ref[2] else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coded-mib", type=int, default=1024)
    ap.add_argument("--flags", type=int, default=100_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pgrc_amd import HufCoder, VarLenDNACoder, synth
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 2
    coder = HufCoder(device=0, block_order=ORDER, table_log=11)
    target = args.coded_mib << 20
    book = next(vu.parse_stream(streams[0])[2] for _, _, streams in vu.load_fixtures() if 0 in streams)
    vl = VarLenDNACoder(book.raw + b"\0", device=0)
    # texts of at most 2 G symbols, coded one by one, until the coded bytes reach the target
    G = min(4 * target, 2_000_000_000)
    words = torch.empty((G + 15) // 16, dtype=torch.int32, device="cuda")
    pieces, have, symbols = [], 0, 0
    while have < target and len(pieces) < 16:
        synth.pg_device(synth.pg_params(G, seed=77 + len(pieces), tandem_every=64), words.data_ptr())
        torch.cuda.synchronize()
        text = unpack_words(torch, words, G)
        pieces.append(vl.encode(text).clone())
        have += int(pieces[-1].numel())
        symbols += G
    varlen_ratio = round(have / symbols, 4)
    d_varlen = torch.cat(pieces)[:target].clone()
    del text, words, pieces
    vl.close()
    res = {"what": "HufCoder (Huffman mode of coder type 5) on the device: two inputs, device to device and from page-locked memory, "
                   "beside a device copy and the reference on one host core",
           "block_order": ORDER, "table_log": 11, "repeats": REPEATS, "varlen_coded_per_symbol": varlen_ratio,
           "varlen": measure(torch, coder, d_varlen)}
    del d_varlen
    flags = (torch.rand(args.flags, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) < 0.5).to(torch.uint8)
    res["flags"] = measure(torch, coder, flags)
    coder.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["varlen"]["round_trip_equal"] and res["flags"]["round_trip_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
