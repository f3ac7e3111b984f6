"""The round skip of the dual kernel (pgrc_amd/csrc/dualkern.h, "Round skip") restated on the CPU for one strand's
query, beside the reference's order.

`query` follows the oracle's restatement of the reference's per-read query (oracle/pgrc_oracle.c, match_read_ex:
CopMEMMatcher.cpp:483-566 with the early-stop rule) seed by seed.  With skip=True it adds the kernel's schedule: when a
round ends and the query goes on, it passes over the seeds between this round and the next one and probes round seeds
only -- every bucket whole, no falses counted, nothing accepted.  A candidate with a count <= limit, or the end of the
seeds, sends it back to the first passed-over seed with the clean rounds it had then; from there it goes on in order
(and may skip again at the next round end).  A query whose clean rounds exceed the limit in skip mode ends.

`match_two_pass` runs the reference's two passes (forward text, then the reverse complement from the forward count) with
that query, so that its positions, strands and counts can be compared with oracle.oracle_match(..., early_stop=True).
The probe counters give the line-saving estimate of the rule (a probed seed is one head line of the dual kernel)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle as orc
from util import revcomp

BUCKET_CAP = 13      # CopMEMMatcher.h:11
TRUNC_BUCKET = 4     # CopMEMMatcher.h:13
NOT_MATCHED_POS = (1 << 64) - 1
NOT_MATCHED_CNT = 255


class Strand:
    """One strand's text and its serial index (pgrc_or_index_build: cumm / positions)."""

    def __init__(self, text, seed_len):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        prm, self.cumm, self.positions = orc.oracle_index(self.text, seed_len)
        self.K, self.k1, self.k2 = prm["K"], prm["k1"], prm["k2"]
        self.mask = prm["hash_size"] - 1
        self.G = self.text.size


def seed_hashes(strand, read):
    """bucket number of every seed s = 0, k2, ... of the read (pgrc_or_copmem_hash)"""
    L = read.size
    buf = C.create_string_buffer(read.tobytes(), L)
    base = C.addressof(buf)
    h = orc.oracle().pgrc_or_copmem_hash
    return [h(strand.K, C.cast(base + s, C.c_char_p)) & strand.mask for s in range(0, L - strand.K + 1, strand.k2)]


class Stats:
    def __init__(self):
        self.probes = 0      # seeds probed (one head line each in the dual kernel)
        self.skipped = 0     # queries that entered skip mode
        self.rewinds = 0


def query(strand, read, hashes, kmax, kmin, cnt, skip, stats):
    """One strand's query of one read; returns (position or NOT_MATCHED_POS, count)."""
    K, k1, k2, G = strand.K, strand.k1, strand.k2, strand.G
    L = read.size
    nseeds = len(hashes)
    limit = kmax if cnt >= kmax else cnt - 1           # :488-489
    head = (L // 8) * 8
    budget = (L + 1 - K) // k2
    rper = (K + k1 * k2 - 1) // (k1 * k2) * k1
    falses = 0
    best = NOT_MATCHED_POS
    i, rq, rclean, rdirty = 0, 0, 0, False
    skipping, resume, rcl_snap, was_skipping = False, 0, 0, False
    while True:
        if i >= nseeds:
            if not skipping:
                break
            skipping, i, rq, rclean, rdirty = False, resume, k1, rcl_snap, False   # the seeds ran out in skip mode
            stats.rewinds += 1
            continue
        stats.probes += 1
        s = i * k2
        lo, hi = int(strand.cumm[hashes[i]]), int(strand.cumm[hashes[i] + 1])
        rewound = False
        if hi > lo:
            trunc = not skipping and budget < falses and hi > lo + TRUNC_BUCKET
            if rq < k1 and (hi - lo >= BUCKET_CAP or trunc):
                rdirty = True
            if trunc:
                hi = lo + TRUNC_BUCKET                     # :510-514
            for j in range(lo, hi):
                sp = int(strand.positions[j])
                if s > sp or sp - s + L > G:               # :517-520
                    continue
                diff = read != strand.text[sp - s:sp - s + L]
                mh = int(np.count_nonzero(diff[:head]))
                m = mh + int(np.count_nonzero(diff[head:]))
                if skipping:
                    if m <= limit:                         # acceptable: back to the passed-over seeds, in order
                        skipping, i, rq, rclean, rdirty = False, resume, k1, rcl_snap, False
                        stats.rewinds += 1
                        rewound = True
                        break
                    continue
                if mh > limit:
                    falses += 1
                    continue
                if m > limit:
                    falses += 2                            # :548-549
                    continue
                cnt, best = m, sp - s
                if m <= kmin:                              # :556-559
                    return best, cnt
                limit = m - 1
        if rewound:
            continue
        # the seed is done: the next one (the early-stop bookkeeping of match_read_ex)
        if rq == k1 - 1:
            rclean += 0 if rdirty else 1
            rdirty = False
        rq = 0 if rq + 1 == rper else rq + 1
        i += 1
        if rclean > limit:
            break
        if skip and rq == k1 and i < nseeds:
            nx = i + rper - k1                             # the next round's first seed
            if not skipping and nx < nseeds:
                skipping, resume, rcl_snap = True, i, rclean
                if not was_skipping:
                    stats.skipped += 1
                    was_skipping = True
            if skipping:
                i, rq = nx, 0
    return best, cnt


def match_two_pass(pg, reads, seed_len, kmax, kmin, skip, strands=None, stats=None):
    """The reference's two passes with `query`; returns (result dict, Stats)."""
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    n, L = reads.shape
    if strands is None:
        strands = (Strand(pg, seed_len), Strand(revcomp(np.ascontiguousarray(pg, dtype=np.uint8)), seed_len))
    stats = stats or Stats()
    G = strands[0].G
    pos = np.full(n, NOT_MATCHED_POS, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint8)
    mism = np.full(n, NOT_MATCHED_CNT, dtype=np.uint8)
    for pas, st in enumerate(strands):
        for r in range(n):
            if mism[r] <= kmin:                            # ReadsMatchers.cpp:430
                continue
            rd = reads[r]
            p, c = query(st, rd, seed_hashes(st, rd), kmax, kmin, int(mism[r]), skip, stats)
            if p != NOT_MATCHED_POS and c < mism[r]:       # :437-447
                pos[r] = G - (p + L) if pas else p
                rc[r] = pas
                mism[r] = c
    return {"pos": pos, "rc": rc, "mism": mism, "matched": int((mism != NOT_MATCHED_CNT).sum())}, stats
