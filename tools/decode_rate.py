"""Rate of the read rebuild on the device (include/pgrc_decode.h).

A C3-size job (100 M x 150 bp over a 1.875 Gbp synthetic pseudogenome, mode c, seed 38, -M 50) is matched and exported on
the device (Pg order, the order made on the device; an old reads list every 200 symbols up to the text end), the unmatched
reads become the LQ text, and the reads are rebuilt in SE, PE and ORD order.  Prints one JSON line: device ms per phase,
bytes, the fraction of 8 TB/s (SE) or of the chip's random 128-byte-line rate (PE / ORD), and the end-to-end rate of SE
rows into pinned host memory against the measured ~57 GB/s device-to-host link.  Every SE row and
every ORD row of a read is compared with the input read; the PE rows of file 1 are compared too.

    python tools/decode_rate.py [--reads N] [--pg-len G] [--out profiles/....json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8e12          # MI355X HBM3E peak
LINE_RATE = 49e9        # random 128-byte lines per second the chip serves
LINK_BPS = 57e9         # measured device-to-host copy rate


def reads_host_parallel(synth, lib, g, pg, rs, n, L, threads=16):
    out = np.empty((n, L), dtype=np.uint8)
    step = (n + threads - 1) // threads

    def part(k):
        a = k * step
        c = min(step, n - a)
        if c > 0:
            lib.pgrc_synth_reads_host(C.byref(g), pg.ctypes.data_as(C.c_void_p), C.byref(rs), a, c,
                                      out[a:a + c].ctypes.data_as(C.c_void_p))
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(threads)))
    return out


def equal_rows(rows, want, block=1 << 20):
    for a in range(0, rows.shape[0], block):
        if not np.array_equal(rows[a:a + block, :-1], want(a, min(a + block, rows.shape[0]))):
            return False
    return bool((rows[:, -1] == ord("\n")).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--pg-len", type=int, default=1_875_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pgrc_amd import MatchContext, PgRCDecoder, synth
    from pgrc_amd._lib import lib
    n, L, G = args.reads, args.read_len, args.pg_len
    t0 = time.time()
    g = synth.pg_params(G, seed=12345)
    pg = synth.pg_host(g)
    reads = reads_host_parallel(synth, lib, g, pg, synth.reads_params(n, L, seed=12345), n, L)
    t_gen = time.time() - t0
    lpos = np.arange(0, G - L + 1, 200, dtype=np.int64)
    if lpos[-1] != G - L:
        lpos = np.append(lpos, G - L)
    h = lpos.size
    loff = np.diff(lpos, prepend=0).astype(np.uint8)
    ctx = MatchContext(L, 38, 50, 0, "c", device=0)
    ctx.set_pg_ascii(pg)
    ctx.set_reads_ascii(reads)
    ctx.init_results()
    ctx.run(True)
    pos, rc, mism, _, matched = ctx.get_results()
    st = ctx.export_pg_order(None, loff, (n + np.arange(h)).astype(np.uint32))
    ctx.close()
    del ctx
    um = np.flatnonzero(mism == 255)
    text = np.concatenate([pg, reads[um].reshape(-1)])
    ne = st["org_idx"].size
    T = ne + um.size

    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    dec.add_list(ne, 0, off=st["off"], rev_comp=st["rev_comp"], mis_cnt=st["mis_cnt"], mis_sym=st["mis_sym"],
                 mis_off=st["mis_rev_off"], mis_sym_form=1)
    dec.add_list(um.size, G, pos=np.arange(um.size, dtype=np.uint64) * L)
    tm_setup = dec.timing()
    org = st["org_idx"].astype(np.int64)
    out = {"what": "read rebuild (pgrc_decode_*) of a C3-size job matched and exported on the device", "reads": n, "read_len": L,
           "pg_len": G, "old_list_entries": h, "matched": int(matched), "rows": int(T), "text_bytes": int(text.size),
           "host_generate_s": round(t_gen, 1), "ms_text_upload": round(tm_setup["ms_text"], 1),
           "ms_lists_device": round(tm_setup["ms_lists_device"], 2)}
    L1 = L + 1
    dbuf = torch.empty(T * L1 + 64, dtype=torch.uint8, device="cuda:0")
    # SE: device rows, then the whole job into pinned host memory (best of two)
    dec.set_order(0)
    ms = []
    for _ in range(3):
        dec.rows_device(0, 0, T, dbuf.data_ptr())
        ms.append(dec.timing()["ms_rows_device"])
    se_ms = min(ms)
    se_bytes = T * L1 + text.size + ne * 8          # rows written, text read once, positions
    pinned = torch.empty(T * L1, dtype=torch.uint8, pin_memory=True)
    rows = pinned.numpy().reshape(T, L1)
    e2e = []
    for _ in range(2):
        dec.rows(0, 0, T, out=rows)
        e2e.append(dec.timing()["ms_rows"])
    def hq_want(a, b):      # a matched read's entry is its read, an old list entry its Pg window
        o = org[a:b]
        w = np.empty((b - a, L), dtype=np.uint8)
        m = o < n
        w[m] = reads[o[m]]
        w[~m] = pg[lpos[o[~m] - n][:, None] + np.arange(L)]
        return w
    ok_hq = equal_rows(rows[:ne], hq_want)
    ok_lq = equal_rows(rows[ne:], lambda a, b: reads[um[a:b]])
    out["se"] = {"ms_device": round(se_ms, 3), "rows_bytes": int(T * L1), "bytes_est": int(se_bytes),
                 "frac_of_8TBps": round(se_bytes / (se_ms * 1e-3) / HBM_BPS, 3),
                 "e2e_ms_pinned": round(min(e2e), 1), "e2e_GBps": round(T * L1 / (min(e2e) * 1e-3) / 1e9, 1),
                 "frac_of_link_57GBps": round(T * L1 / (min(e2e) * 1e-3) / LINK_BPS, 3),
                 "rows_equal_reads": bool(ok_hq and ok_lq)}
    # PE: rlIdxOrder by original index (reads first, then the old list's entries)
    rl_of_org = np.empty(T, dtype=np.uint32)
    rl_of_org[org] = np.arange(ne, dtype=np.uint32)
    rl_of_org[um] = ne + np.arange(um.size, dtype=np.uint32)
    dec.set_order(1, T, rl_idx_order=rl_of_org)
    pe_ms = 0.0
    for p in range(2):
        npr = dec.row_count(p)
        dec.rows_device(p, 0, npr, dbuf.data_ptr())
        pe_ms += dec.timing()["ms_rows_device"]
    n1 = dec.row_count(0)
    f1 = dec.rows(0, 0, min(n1, 2_000_000))
    o1 = np.arange(0, 2 * f1.shape[0], 2)
    ok_pe = equal_rows(f1[o1 < n], lambda a, b: reads[o1[o1 < n][a:b]])
    lines = T * ((L + 15 + 127) // 128 + 1)
    out["pe"] = {"ms_device": round(pe_ms, 3), "rows_bytes": int(T * L1), "GBps_written": round(T * L1 / (pe_ms * 1e-3) / 1e9, 1),
                 "window_lines_est": int(lines), "frac_of_random_line_rate": round(lines / (pe_ms * 1e-3) / LINE_RATE, 3),
                 "file1_rows_checked_equal_reads": bool(ok_pe)}
    dec.close()
    # ORD: the original-order export is not made here; the same HQ list read by rank: orgIdx2PgPos of the matched reads
    # in original order needs their entries in that order -- made by a stable sort of the Pg-order list by index
    ordr = np.argsort(org, kind="stable")
    o2p = np.zeros(T, dtype=np.uint64)
    o2p[org] = np.where(org < n, pos[np.minimum(org, n - 1)], lpos[np.maximum(org - n, 0)]).astype(np.uint64)
    o2p[um] = G + np.arange(um.size, dtype=np.uint64) * L
    cnt = st["mis_cnt"].astype(np.int64)
    inv = np.empty(ne, dtype=np.int64)
    inv[ordr] = np.arange(ne)
    sel = np.argsort(inv[np.repeat(np.arange(ne), cnt)], kind="stable")     # mismatches in the entries' new order
    dec = PgRCDecoder(L, device=0)
    dec.set_text(text)
    dec.add_list(ne, 0, rev_comp=st["rev_comp"][ordr], mis_cnt=st["mis_cnt"][ordr], mis_sym=st["mis_sym"][sel],
                 mis_off=st["mis_rev_off"][sel], mis_sym_form=1)
    dec.add_list(um.size, G, pos=np.arange(um.size, dtype=np.uint64) * L)
    dec.set_order(2, T, org_idx_to_pos=o2p)
    dec.rows_device(0, 0, T, dbuf.data_ptr())
    ord_ms = dec.timing()["ms_rows_device"]
    rows = pinned.numpy().reshape(T, L1)
    dec.rows(0, 0, T, out=rows)
    ok_ord = equal_rows(rows[:n], lambda a, b: reads[a:b])
    out["ord"] = {"ms_device": round(ord_ms, 3), "GBps_written": round(T * L1 / (ord_ms * 1e-3) / 1e9, 1),
                  "window_lines_est": int(lines), "frac_of_random_line_rate": round(lines / (ord_ms * 1e-3) / LINE_RATE, 3),
                  "rows_of_reads_equal_reads": bool(ok_ord)}
    dec.close()
    out["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = out["se"]["rows_equal_reads"] and out["pe"]["file1_rows_checked_equal_reads"] and out["ord"]["rows_of_reads_equal_reads"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
