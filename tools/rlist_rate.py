"""The HQ reads list's way through the second half of the encoder, on both routes in one process (include/pgrc_readslist.h;
DESIGN.md section 4.20): assembly result -> export -> archive form -> pair order.

--reads reads of 150 bp split 80 / 15 / 5 % into HQ / LQ / N.  The HQ list has one entry per HQ read (offsets below 8, a random
permutation's indexes); the matcher holds the LQ + N reads as random packed rows over a random text of the list's span, and its
results are set, not searched (pgrc_match_set_results: 60 % matched at sorted random positions, 0 .. 3 mismatches each) -- the
export's kernels then find that many mismatches per read, as they would after a search.  Per seam, the parent's route through
the existing entry points and the resident route through pgrc_rlist, wall time around calls that are complete on return,
medians of --repeats after a warm-up, and the bytes that cross the link on each:
  assembly   the copy of org_idx and off to page-locked host memory that pgrc_asm_run makes (6 bytes per entry), against the
             device copy of pgrc_rlist_from_assembly; both are timed as plain copies of those bytes, which is also the yardstick
             for every other device-to-device copy of the object (bytes_device_copy of its timing)
  export     pgrc_match_export_pg_order against pgrc_rlist_export_pg_order (the reads' original indexes from host memory on both)
  archive    pgrc_list_archive_encode on the streams the export returned against pgrc_rlist_archive_encode
  pair_order pgrc_pairorder_encode on the three host arrays against pgrc_rlist_pair_order
Prints one JSON object and writes it to --out.  Needs the device: there is no other way to take these numbers.

--ord times the order-preserving mode's way instead, on the same split and the same lists and matcher:
  export     pgrc_match_export_original_order (seven streams of one entry per original read down into pageable memory) against
             pgrc_rlist_export_original_order into a second list (the reads' original indexes from host memory on both)
  archive    pgrc_list_archive_encode on the streams the export returned against pgrc_rlist_archive_encode_ord
  positions  the three lists' off and org_idx brought down (pgrc_rlist_download) and orgIdx2PgPos scattered with numpy and
             narrowed to four bytes, against pgrc_rlist_positions

    python tools/rlist_rate.py [--ord] [--reads R] [--repeats N] [--out profiles/rlist_rate.json | profiles/rlist_rate_ord.json]
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


def stat(v):
    v = sorted(float(x) for x in v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def timed(fn, *a, **kw):
    t0 = time.perf_counter()
    r = fn(*a, **kw)
    return r, (time.perf_counter() - t0) * 1e3


def positions_host(T, lists, bases, read_org, pos, matched):
    """the caller's way to orgIdx2PgPos without pgrc_rlist_positions: every list's off and org_idx down, three scatters"""
    arr = np.full(T, np.uint64(2**64 - 1), dtype=np.uint64)
    down = 0
    for l, base in zip(lists, bases):
        st = l.download()
        down += int(l.timing()["bytes_down"])
        arr[st["org_idx"]] = np.uint64(base) + np.cumsum(st["off"], dtype=np.uint64)
    arr[read_org[matched]] = pos[matched]
    return arr.astype(np.uint32), down


def main_ord(args, ctx, dec, hq, rest, read_org, pos, matched, R, n_hq, n_rest, G):
    """the ORD way on both routes; the lists and the matcher are main()'s"""
    from pgrc_amd import ReadsList
    lq_len = L
    bases = (0, G, G + lq_len)
    out_list = ReadsList(0)
    seams = {k: {"host_ms": [], "resident_ms": []} for k in ("export", "archive", "positions")}
    dev = {k: [] for k in seams}
    for rep in range(args.repeats + 1):
        exp, ms_eh = timed(ctx.export_original_order, read_org, R, False, False, True)
        _, ms_er = timed(out_list.export_original_order, ctx, R, read_org, None, False, False, True)
        t_exp = out_list.timing()
        _, ms_ah = timed(dec.list_archive_encode, exp["mis_cnt"], exp["mis_sym"], exp["mis_rev_off"])
        arch, ms_ar = timed(out_list.archive_encode_ord, False)
        t_arch = out_list.timing()
        (want, pos_down), ms_ph = timed(positions_host, R, [hq] + rest, bases, read_org, pos, matched)
        got, ms_pr = timed(hq.positions, R, 4, rest[0], rest[1], G, lq_len, ctx, read_org)
        t_pos = hq.timing()
        assert np.array_equal(got, want)
        if rep:                             # (the first round is the warm-up)
            for k, h, r, t in (("export", ms_eh, ms_er, t_exp), ("archive", ms_ah, ms_ar, t_arch), ("positions", ms_ph, ms_pr, t_pos)):
                seams[k]["host_ms"].append(h)
                seams[k]["resident_ms"].append(r)
                dev[k].append(t)
    ne, nm = int(exp["org_idx"].size), int(exp["mis_sym"].size)
    out = {"mode": "ord", "reads": R, "read_len": L, "repeats": args.repeats, "hq_entries": n_hq, "matcher_reads": n_rest, "matched": int(matched.sum()),
           "entries": ne, "mismatches": nm, "text_symbols": G, "pos_width": 4, "seams": {}}
    bytes_host = {"export": {"up": 4 * n_rest, "down": 7 * ne + 2 * nm},
                  "archive": {"up": ne + 2 * nm, "down": int(dec.list_archive_timing()["bytes_down"])},
                  "positions": {"up": 0, "down": pos_down}}
    for k, v in seams.items():
        t = dev[k][-1]
        o = {"host_route": {"ms": stat(v["host_ms"]), "bytes": bytes_host[k]},
             "resident_route": {"ms": stat(v["resident_ms"]), "bytes": {"up": int(t["bytes_up"]), "down": int(t["bytes_down"]), "device_copy": int(t["bytes_device_copy"])},
                                "device_ms": {p: stat([x[p] for x in dev[k]]) for p in ("ms_fetch_device", "ms_build_device", "ms_pack_device")},
                                "call_ms": stat([x["ms_call"] for x in dev[k]])}}
        o["host_over_resident"] = round(o["host_route"]["ms"]["median"] / max(o["resident_route"]["ms"]["median"], 1e-6), 2)
        out["seams"][k] = o
    out["link_bytes"] = {"host_route": sum(sum(b.values()) for b in bytes_host.values()),
                         "resident_route": sum(o["resident_route"]["bytes"]["up"] + o["resident_route"]["bytes"]["down"] for o in out["seams"].values())}
    out["archive_block_bytes"] = int(arch["block_bytes"])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ord", action="store_true", help="the order-preserving mode's way (export, archive block, positions)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rlist_rate_ord.json" if args.ord else "rlist_rate.json")
    import torch
    from pgrc_amd import MatchContext, PgRCDecoder, ReadsList
    rng = np.random.default_rng(1)
    R = args.reads - args.reads % 2
    n_hq, n_rest = int(R * 0.8), R - int(R * 0.8)
    perm = rng.permutation(R).astype(np.uint32)
    hq_off = rng.integers(0, 8, size=n_hq).astype(np.uint8)
    hq_org = perm[:n_hq]
    G = int(hq_off.sum(dtype=np.int64)) + L
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=G)]
    rows = rng.integers(0, 256, size=(n_rest, (L + 3) // 4), dtype=np.uint8)
    matched = rng.random(n_rest) < 0.6
    pos = np.full(n_rest, np.uint64(2**64 - 1), dtype=np.uint64)
    pos[matched] = rng.integers(0, G - L, size=int(matched.sum())).astype(np.uint64)
    mism = np.where(matched, rng.integers(0, 4, size=n_rest), 255).astype(np.uint8)
    rc = (rng.random(n_rest) < 0.5).astype(np.uint8) * matched
    read_org = perm[n_hq:]
    n_lq = int(n_rest * 0.75)
    left = [read_org[:n_lq][~matched[:n_lq]], read_org[n_lq:][~matched[n_lq:]]]
    ctx = MatchContext(L, 38, 3, 0, "c", device=0)
    ctx.set_pg_ascii(text)
    ctx.set_reads_packed(rows, n_rest)
    ctx.init_results()
    ctx.set_results(pos, rc, mism)
    del text, rows
    dec = PgRCDecoder(L, device=0)
    rest = []
    for org in left:
        l = ReadsList(0)
        l.set_host(np.zeros(org.size, np.uint8), org)
        rest.append(l)
    hq = ReadsList(0)
    if args.ord:
        hq.set_host(hq_off, hq_org)
        return main_ord(args, ctx, dec, hq, rest, read_org, pos, matched, R, n_hq, n_rest, G)
    seams = {k: {"host_ms": [], "resident_ms": []} for k in ("assembly", "export", "archive", "pair_order")}
    dev = {k: [] for k in ("export", "archive", "pair_order")}
    # the assembly seam and the yardstick: 6 bytes per entry down to page-locked memory, or device to device
    d_src = torch.empty(6 * n_hq, dtype=torch.uint8, device="cuda").random_(0, 256)
    d_dst = torch.empty_like(d_src)
    h_dst = torch.empty(6 * n_hq, dtype=torch.uint8).pin_memory()
    exp = None
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        _, ms_h = timed(lambda: (h_dst.copy_(d_src, non_blocking=True), torch.cuda.synchronize()))
        _, ms_d = timed(lambda: (d_dst.copy_(d_src, non_blocking=True), torch.cuda.synchronize()))
        # export
        exp, ms_eh = timed(ctx.export_pg_order, None, hq_off, hq_org, None, read_org, False, True)
        hq.set_host(hq_off, hq_org)
        _, ms_er = timed(hq.export_pg_order, ctx, None, read_org, None, False, True)
        t_exp = hq.timing()
        # archive form
        _, ms_ah = timed(dec.list_archive_encode, exp["mis_cnt"], exp["mis_sym"], exp["mis_rev_off"])
        arch, ms_ar = timed(hq.archive_encode, False, False)
        t_arch = hq.timing()
        # pair order
        _, ms_ph = timed(dec.compressReadsOrder, [exp["org_idx"]] + left, 0)
        po_down = dec.pairorder_timing()["bytes_down"]
        _, ms_pr = timed(ReadsList.pair_order, [hq] + rest, 0)
        t_po = hq.timing()
        if rep:                             # (the first round is the warm-up)
            for k, h, r in (("assembly", ms_h, ms_d), ("export", ms_eh, ms_er), ("archive", ms_ah, ms_ar), ("pair_order", ms_ph, ms_pr)):
                seams[k]["host_ms"].append(h)
                seams[k]["resident_ms"].append(r)
            for k, t in (("export", t_exp), ("archive", t_arch), ("pair_order", t_po)):
                dev[k].append(t)
    ne, nm = int(exp["org_idx"].size), int(exp["mis_sym"].size)
    out = {"reads": R, "read_len": L, "repeats": args.repeats, "hq_entries": n_hq, "matcher_reads": n_rest, "matched": int(matched.sum()),
           "merged_entries": ne, "mismatches": nm, "text_symbols": G, "seams": {}}
    bytes_host = {"assembly": {"down": 6 * n_hq, "up": 0},
                  "export": {"up": 6 * n_hq + 4 * n_rest, "down": 7 * ne + 2 * nm},
                  "archive": {"up": ne + 2 * nm, "down": int(dec.list_archive_timing()["bytes_down"])},
                  "pair_order": {"up": 4 * R, "down": int(po_down)}}
    bytes_res = {"assembly": {"up": 0, "down": 0, "device_copy": 6 * n_hq},
                 "export": {"up": int(t_exp["bytes_up"]), "down": int(t_exp["bytes_down"]), "device_copy": int(t_exp["bytes_device_copy"])},
                 "archive": {"up": int(t_arch["bytes_up"]), "down": int(t_arch["bytes_down"]), "device_copy": int(t_arch["bytes_device_copy"])},
                 "pair_order": {"up": int(t_po["bytes_up"]), "down": int(t_po["bytes_down"]), "device_copy": int(t_po["bytes_device_copy"])}}
    for k, v in seams.items():
        o = {"host_route": {"ms": stat(v["host_ms"]), "bytes": bytes_host[k]}, "resident_route": {"ms": stat(v["resident_ms"]), "bytes": bytes_res[k]}}
        o["host_over_resident"] = round(o["host_route"]["ms"]["median"] / max(o["resident_route"]["ms"]["median"], 1e-6), 2)
        if k in dev:
            o["resident_route"]["device_ms"] = {p: stat([t[p] for t in dev[k]]) for p in ("ms_fetch_device", "ms_build_device", "ms_pack_device")}
        out["seams"][k] = o
    out["memcpy_d2d_GBps"] = round(2 * 6 * n_hq / seams["assembly"]["resident_ms"][len(seams["assembly"]["resident_ms"]) // 2] / 1e6, 1)
    tot_h = sum(sum(b.values()) for b in bytes_host.values())
    tot_r = sum(b["up"] + b["down"] for b in bytes_res.values())
    out["link_bytes"] = {"host_route": tot_h, "resident_route": tot_r}
    out["archive_block_bytes"] = int(arch["block_bytes"])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
