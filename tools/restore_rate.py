"""Rate of the restore of the matched pseudogenomes on the device (pgrc_decode_set_mapped_text).

A C3-size input: a synthetic 1.875 Gbp HQ (pgrc_amd.synth) that carries planted reverse-complement copies, some of them
copies of copies, and a 60 Mbp LQ of HQ stretches on both strands between random stretches.  The Pg-vs-Pg matches come
from the device matcher (CopMEMMatcher, pgrc_mem_*), tests/pgmap_util's restatement of markAndRemoveExactMatches turns
them into the mapped text and its streams, and the device restores them.  The restored text's digest is compared with
the original's.  Prints one JSON line: device ms of each stage, the literal pass against a device-to-device copy of the
same bytes timed in this process, and the whole call from pageable and from pinned host memory against
pgrc_decode_set_text of the restored text from the same memory.

    python tools/restore_rate.py [--pg-len G] [--lq-len N] [--out profiles/....json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pgmap_util as pu  # noqa: E402

HBM_BPS = 6e12          # the sustained HBM rate the issue's estimate assumes (an estimate, not a measurement)


def digest(a) -> str:
    return hashlib.sha256(memoryview(np.ascontiguousarray(a, dtype=np.uint8))).hexdigest()[:16]


def plant(pg, rng, copies, depth):
    """reverse-complement copies of random stretches, each copy copied again `depth` - 1 times further on"""
    G = pg.size
    for _ in range(copies):
        ln = int(rng.integers(300, 6000))
        at = int(rng.integers(0, G // 2))
        for _ in range(depth):
            if at + 2 * ln >= G - ln:
                break
            d = int(rng.integers(at + ln, min(G - ln, at + ln + G // (2 * depth))))
            pg[d:d + ln] = pu.revcomp_np(pg[at:at + ln])
            at = d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pg-len", type=int, default=1_875_000_000)
    ap.add_argument("--lq-len", type=int, default=60_000_000)
    ap.add_argument("--target-len", type=int, default=45)
    ap.add_argument("--copies", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pgrc_amd import CopMEMMatcher, PgRCDecoder, synth

    t0 = time.time()
    G, GL, tl = args.pg_len, args.lq_len, args.target_len
    g = synth.pg_params(G, seed=77, tandem_every=64)
    hq = synth.pg_host(g)
    rng = np.random.default_rng(77)
    plant(hq, rng, args.copies, 3)
    lq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=GL)
    for _ in range(GL // 3000):
        ln = int(rng.integers(100, 2000))
        s, d = int(rng.integers(0, G - ln)), int(rng.integers(0, GL - ln))
        lq[d:d + ln] = pu.revcomp_np(hq[s:s + ln]) if rng.random() < 0.7 else hq[s:s + ln]
    nn = np.zeros(0, np.uint8)
    t_gen = time.time() - t0

    t1 = time.time()
    tm = CopMEMMatcher(hq, tl, device=0)
    mapped, lens, offs, lns, found = pu.map_all(hq, lq, nn, lambda s, q, dis, rc: tm.matchTexts(q, dis, rc), tl)
    tm.close()
    t_map = time.time() - t1
    mapped = np.frombuffer(mapped, np.uint8)
    want = {"hq": digest(hq), "lq": digest(lq)}

    dec = PgRCDecoder(150, device=0)
    runs = []
    for _ in range(3):                                   # pageable; the first call also sizes the pooled buffers
        c0 = time.perf_counter()
        dec.restoreMatchedPgs(mapped, lens, G, offs, lns)
        runs.append(((time.perf_counter() - c0) * 1e3, dec.restore_timing()))
    ms_pageable = min(r[0] for r in runs[1:])
    timing = runs[-1][1]
    out = dec.text()
    got = {"hq": digest(out[:G]), "lq": digest(out[G:])}
    total = out.size
    # from pinned memory
    pin = torch.empty(mapped.size, dtype=torch.uint8).pin_memory()
    pin.numpy()[:] = mapped
    pin_runs = []
    for _ in range(3):
        c0 = time.perf_counter()
        dec.restoreMatchedPgs(pin.numpy(), lens, G, offs, lns)
        pin_runs.append((time.perf_counter() - c0) * 1e3)
    ms_pinned = min(pin_runs[1:])
    # set_text of the restored text from the same kinds of memory
    st_page = []
    for _ in range(3):
        c0 = time.perf_counter()
        dec.set_text(out)
        st_page.append((time.perf_counter() - c0) * 1e3)
    pin_out = torch.empty(total, dtype=torch.uint8).pin_memory()
    pin_out.numpy()[:] = out
    st_pin = []
    for _ in range(3):
        c0 = time.perf_counter()
        dec.set_text(pin_out.numpy())
        st_pin.append((time.perf_counter() - c0) * 1e3)
    dec.close()
    # a device-to-device copy of the literal bytes (the mapped text minus its marks), timed with events
    lit_bytes = int(mapped.size - sum(timing["marks"]))
    a = torch.empty(lit_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    d2d = []
    for _ in range(5):
        ev0.record()
        b.copy_(a)
        ev1.record()
        torch.cuda.synchronize()
        d2d.append(ev0.elapsed_time(ev1))
    ms_d2d = min(d2d[1:])
    del a, b

    res = {
        "what": "restore of the matched pseudogenomes (pgrc_decode_set_mapped_text) at C3 size, matches from the device matcher",
        "pg_len": G, "lq_len": GL, "target_len": tl, "copies_planted": args.copies,
        "mapped_bytes": [int(x) for x in lens], "restored_bytes": int(total),
        "raw_matches": [int(f.shape[0]) for f in found],
        "marks": timing["marks"], "matched": timing["matched"], "passes": timing["passes"],
        "ms_parse_device": round(timing["ms_parse_device"], 3),
        "ms_literals_device": round(timing["ms_literals_device"], 3),
        "ms_matches_device": round(timing["ms_matches_device"], 3),
        "ms_device_total": round(timing["ms_parse_device"] + timing["ms_literals_device"] + timing["ms_matches_device"], 3),
        "ms_d2d_copy_of_literal_bytes": round(ms_d2d, 3),
        "literals_over_d2d": round(timing["ms_literals_device"] / ms_d2d, 2),
        "ms_estimate_2G_bytes_at_6TBps": round(2 * total / HBM_BPS * 1e3, 3),
        "call_ms_pageable": round(ms_pageable, 1), "upload_ms_pageable": round(runs[-1][1]["ms_upload"], 1),
        "call_ms_pinned": round(ms_pinned, 1),
        "set_text_ms_pageable": round(min(st_page[1:]), 1), "set_text_ms_pinned": round(min(st_pin[1:]), 1),
        "digest_want": want, "digest_got": got, "equal": want == got,
        "host_generate_s": round(t_gen, 1), "host_match_and_map_s": round(t_map, 1),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
