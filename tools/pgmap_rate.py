"""Rate of the mapping of matched pseudogenomes on the device (pgrc_mem_mark_and_remove).

The inputs of tools/restore_rate.py at C3 size: a synthetic 1.875 Gbp HQ (pgrc_amd.synth) with planted chains of
reverse-complement copies and a 60 Mbp LQ of HQ stretches on both strands between random stretches.  Per part the device
matcher finds the matches (CopMEMMatcher.matchTexts), which leaves the destination packed in HBM, and
markAndRemoveExactMatches maps it.  Recorded per part: the device time by phase (normalise + sort, path, streams, text),
the download, the whole call into a pageable and into a page-locked buffer (five repeats after a warm-up: median, min,
max), the digest of the mapped text and the sizes of its two streams.  Once, outside the timed region, the mapped parts
joined as tests/pgmap_util.join_parts joins them go through pgrc_decode_set_mapped_text: the restored HQ | LQ | N must have
the original texts' digests.  Prints one JSON line.

    python tools/pgmap_rate.py [--pg-len G] [--lq-len N] [--out profiles/pgmap_rate_c3.json]
"""
import argparse
import hashlib
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
from restore_rate import digest, plant  # noqa: E402

REPEATS = 5
PHASES = ("ms_sort", "ms_path", "ms_streams", "ms_text", "ms_download")


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def timed_calls(tm, found, out):
    """a warm-up, then REPEATS calls into `out` -> the last result, the calls' ms, the phases' ms"""
    res = tm.markAndRemoveExactMatches(found, None, out)
    calls, phases = [], {k: [] for k in PHASES}
    for _ in range(REPEATS):
        c0 = time.perf_counter()
        res = tm.markAndRemoveExactMatches(found, None, out)
        calls.append((time.perf_counter() - c0) * 1e3)
        ms = tm.mapping_timing()
        for k in PHASES:
            phases[k].append(ms[k])
    return res, calls, phases


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
    hq = synth.pg_host(synth.pg_params(G, seed=77, tandem_every=64))
    rng = np.random.default_rng(77)
    plant(hq, rng, args.copies, 3)
    lq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=GL)
    for _ in range(GL // 3000):
        ln = int(rng.integers(100, 2000))
        s, d = int(rng.integers(0, G - ln)), int(rng.integers(0, GL - ln))
        lq[d:d + ln] = pu.revcomp_np(hq[s:s + ln]) if rng.random() < 0.7 else hq[s:s + ln]
    t_gen = time.time() - t0
    want = {"hq": digest(hq), "lq": digest(lq)}

    tm = CopMEMMatcher(hq, tl, device=0)
    pageable = np.empty(G, dtype=np.uint8)
    pinned = torch.empty(G, dtype=torch.uint8).pin_memory().numpy()
    parts, report = {}, {}
    for name, dest, dis in (("lq", lq, False), ("hq", hq, True)):
        c0 = time.perf_counter()
        found = tm.matchTexts(pu.revcomp_np(dest), dis, True)
        ms_match = (time.perf_counter() - c0) * 1e3
        res, calls_page, phases = timed_calls(tm, found, pageable[:dest.size])
        res_pin, calls_pin, phases_pin = timed_calls(tm, found, pinned[:dest.size])
        mapped, off, lens, info = res_pin
        assert res[0].tobytes() == mapped.tobytes()
        parts[name] = (mapped.tobytes(), off.tobytes(), lens.tobytes())
        report[name] = {
            "dest_len": int(dest.size), "raw_matches": int(found.shape[0]), "unique_matches": int(info["unique_matches"]),
            "marks": int(info["marks"]), "matched_symbols": int(info["matched_symbols"]), "mapped_len": int(mapped.size),
            "map_off_bytes": int(off.size), "map_len_bytes": int(lens.size), "mapped_digest": digest(mapped),
            "ms_match_texts_call": round(ms_match, 1),
            "device_ms": {k: spread(phases_pin[k]) for k in PHASES[:4]},
            "download_ms_pageable": spread(phases["ms_download"]), "download_ms_pinned": spread(phases_pin["ms_download"]),
            "call_ms_pageable": spread(calls_page), "call_ms_pinned": spread(calls_pin),
        }
    tm.close()

    # the round trip, once, outside the timed region
    mapped, mlens, offs, lns = pu.join_parts([parts["hq"], parts["lq"], (b"", b"", b"")])
    dec = PgRCDecoder(150, device=0)
    dec.restoreMatchedPgs(np.frombuffer(mapped, np.uint8), mlens, G, offs, lns)
    out = dec.text()
    got = {"hq": digest(out[:G]), "lq": digest(out[G:])}
    lengths = [int(x) for x in dec.text_lengths()]
    dec.close()

    res = {
        "what": "markAndRemoveExactMatches on the device (pgrc_mem_mark_and_remove) at C3 size, matches from the device matcher",
        "pg_len": G, "lq_len": GL, "target_len": tl, "copies_planted": args.copies, "repeats": REPEATS,
        "parts": report,
        "round_trip": {"restored_lengths": lengths, "digest_want": want, "digest_got": got, "equal": want == got},
        "host_generate_s": round(t_gen, 1),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["round_trip"]["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
