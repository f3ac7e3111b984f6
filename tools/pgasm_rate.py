"""Rate of the assembly of a pseudogenome from the overlap graph on the device (pgrc_asm_run).

A generated case of --reads reads of 150 bp over ACGT: chains of about 1000 reads, shifts with a mean of 19 (one read in
twenty a duplicate of the one before), one chain in fifty closed to a cycle, read ids shuffled.  The whole call is timed
after a warm-up, several times, with the input and the text's destination in pageable and in page-locked host memory;
device times are the library's HIP-event figures.  The text is checked against the chains' texts in the order of their
heads.  Prints one JSON object: per phase the median and the spread of the repeats.

    python tools/pgasm_rate.py [--reads R] [--repeats N] [--out profiles/pgasm_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 150
PHASES = ("ms_checks_device", "ms_cycles_device", "ms_rank_device", "ms_lists_device", "ms_text_device")


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def generate(R, seed):
    """-> rows, next_read, overlap, the expected text (without the cuts' effect on it: a cycle's text is its circle from the read
    after its largest id on) and the cycles' count"""
    rng = np.random.default_rng(seed)
    nch = max(1, R // 1000)
    bounds = np.sort(rng.choice(np.arange(1, R), size=nch - 1, replace=False)) if nch > 1 else np.zeros(0, np.int64)
    first = np.concatenate(([0], bounds)).astype(np.int64)          # the first read of every chain, walk order
    last = np.concatenate((bounds, [R])).astype(np.int64) - 1
    cyc = rng.random(nch) < 0.02
    shift = np.minimum(rng.geometric(1.0 / 20.0, size=R), L).astype(np.int64)
    shift[rng.random(R) < 0.05] = 0
    shift[last[~cyc]] = L
    shift[last[cyc]] = np.maximum(shift[last[cyc]], 1)
    start = np.cumsum(shift) - shift
    seg0, seg1 = start[first], start[last] + shift[last]            # the text of chain c: [seg0, seg1); a cycle's is circular
    tlen = seg1 - seg0
    chain_of = np.repeat(np.arange(nch), last - first + 1)
    codes = rng.integers(0, 4, size=int(seg1[-1]), dtype=np.uint8)
    ids = (rng.permutation(R) + 1).astype(np.uint32)
    rows = np.empty((R, (L + 3) // 4), dtype=np.uint8)
    w = np.array([64, 16, 4, 1], dtype=np.uint8)
    for at in range(0, R, 1 << 20):
        j = np.arange(at, min(R, at + (1 << 20)))
        c = chain_of[j]
        rel = (start[j] - seg0[c])[:, None] + np.arange(L + 2)[None, :]
        rel = np.where(cyc[c][:, None], rel % tlen[c][:, None], np.minimum(rel, tlen[c][:, None] - 1))
        sym = codes[seg0[c][:, None] + rel]
        sym[:, L:] = 0
        rows[ids[j] - 1] = (sym.reshape(j.size, -1, 4) * w).sum(axis=2, dtype=np.uint8)
    nx = np.zeros(R + 1, dtype=np.uint32)
    ov = np.zeros(R + 1, dtype=np.uint8)
    succ = np.arange(R) + 1
    succ[last] = np.where(cyc, first, -1)
    has = succ >= 0
    nx[ids[has]] = ids[succ[has]]
    ov[ids] = L - shift
    ov[ids[last[~cyc]]] = 0
    # the expected text: chains by their head's id; a cycle is cut at its largest id, its head is the read after that one
    head = first.copy()
    rot = np.zeros(nch, dtype=np.int64)
    for c in np.flatnonzero(cyc):
        m = first[c] + int(np.argmax(ids[first[c]:last[c] + 1]))
        head[c] = first[c] if m == last[c] else m + 1
        rot[c] = start[head[c]] - seg0[c]
    parts = []
    lost = 0
    for c in np.argsort(ids[head], kind="stable"):
        seg = codes[seg0[c]:seg1[c]]
        if cyc[c]:
            m = last[c] if head[c] == first[c] else head[c] - 1
            lost += L - shift[m]
            seg = np.resize(np.roll(seg, -rot[c]), tlen[c] + L - shift[m])      # the cut read is written out whole
        parts.append(seg)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[np.concatenate(parts)]
    return rows, nx, ov, text, int(cyc.sum()), int(lost)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pgrc_amd import PgAssembler

    R = args.reads
    t0 = time.time()
    rows, nx, ov, text, cycles, lost = generate(R, 2026)
    t_gen = time.time() - t0
    asm = PgAssembler(device=0)
    res = {"what": "pgrc_asm_run, 150 bp over ACGT, one context", "reads": R, "read_len": L, "mean_shift": round(text.size / R, 2), "chains": max(1, R // 1000),
           "cycles": cycles, "pg_len": int(text.size), "repeats": args.repeats}

    def pinned(a):
        t = torch.from_numpy(a).pin_memory()
        return t, t.numpy()

    keep = [pinned(a) for a in (rows, nx, ov)]
    inputs = {"pageable": (rows, nx, ov), "page_locked": tuple(k[1] for k in keep)}
    tdst = {"pageable": np.empty(text.size, dtype=np.uint8), "page_locked": pinned(np.empty(text.size, dtype=np.uint8))[1]}
    for kind in ("pageable", "page_locked"):
        runs = []
        for _ in range(args.repeats + 1):                       # (the first call sizes the buffers)
            c0 = time.perf_counter()
            out = asm.run(*inputs[kind], L, 4)
            c1 = time.perf_counter()
            got = asm.text(out=tdst[kind])
            c2 = time.perf_counter()
            runs.append(dict(asm.timing(), wall_run=(c1 - c0) * 1e3, wall_text=(c2 - c1) * 1e3))
        runs = runs[1:]
        assert out["pg_len"] == text.size and out["cycles"] == cycles and out["overlap_lost"] == lost, (out["pg_len"], text.size, out["cycles"], cycles)
        assert got.tobytes() == text.tobytes(), "the device's text differs from the chains' texts"
        r = {k: stat(x[k] for x in runs) for k in PHASES}
        r["ms_device_total"] = stat(sum(x[k] for k in PHASES) for x in runs)
        r.update(ms_upload_host=stat(x["ms_upload"] for x in runs), ms_download_host=stat(x["ms_download"] for x in runs),
                 ms_call=stat(x["ms_call"] for x in runs), ms_python_run=stat(x["wall_run"] for x in runs),
                 ms_text_to_host=stat(x["wall_text"] for x in runs), passes_cycles=int(runs[0]["passes_cycles"]),
                 passes_rank=int(runs[0]["passes_rank"]), bytes_up=int(runs[0]["bytes_up"]), bytes_down=int(runs[0]["bytes_down"]))
        res[kind] = r
    asm.close()
    res["host_generate_s"] = round(t_gen, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
