#!/usr/bin/env python3
"""Golden fixtures of the edits of the divided read sets (include/pgrc_readsets.h), made by the REAL reference compiled in the
build container (oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, puts FASTQ records
behind the reference's iterator interface, lets the reference's own getQualityDivisionBasedReadsSets divide them (the symbol the
recipe under oracle/ keeps as pgrc_ref_divide_quality_original), then calls moveLqReadsFromHqReadsSetsToLqReadsSets,
generateHqReadsIndexesMapping, removeReadsFromLqReadsSet and removeReadsFromNReadsSet as pgrc-encoder.cpp:367-372 does, and
dumps the packed rows and the mappings before and after.  Fixtures are data only.  The records are made here so that every
read's set is known in advance (an N, or a '#' at the position the simplified suffix rule tests), which lets a case place the
sets' indexes where it wants them; what a case stands for is asserted against the reference's own output.

    python tests/golden/make_golden_rsets.py      # needs the reference tree (run `make -C oracle ref` first)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rsets_util as ru  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")
ERROR_LIMIT = 0.05
HQ, LQ, N, MOVED = 0, 1, 2, 3       # a read's plan: its set, and whether the move takes it out of the HQ set

DRIVER = r"""
#include <chrono>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "readsset/DividedPCLReadsSets.h"
using namespace std;
using namespace PgTools;
extern "C" DividedPCLReadsSets *pgrc_ref_divide_quality_original(ReadsSourceIteratorTemplate<uint_read_len_max> *readsIt, uint_read_len_max readLength,
                                                                  double error_limit, bool simplified_suffix_mode, bool separateNReadsSet, bool nReadsLQ);
static void wr(const string &p, const void *d, size_t n) { ofstream f(p, ios::binary); f.write((const char *) d, n); }
static string rd(const string &p) { ifstream f(p, ios::binary); stringstream ss; ss << f.rdbuf(); return ss.str(); }
struct Records : ReadsSourceIteratorTemplate<uint_read_len_max> {
    string rows, quals, read, qual;
    size_t L, n;
    long at = -1;
    Records(const string &r, const string &q, size_t L_) : rows(r), quals(q), L(L_), n(r.size() / L_) {}
    bool moveNext() override {
        if (at + 1 >= (long) n) return false;
        at++;
        read = rows.substr(at * L, L);
        qual = quals.substr(at * L, L);
        return true;
    }
    string &getRead() override { return read; }
    string &getQualityInfo() override { return qual; }
    uint_read_len_max getReadLength() override { return (uint_read_len_max) L; }
    void rewind() override { at = -1; }
    IndexesMapping *retainVisitedIndexesMapping() override { return new DirectMapping((uint_reads_cnt_max) n); }
};
static bool timing = false;      // argv[5] = "time": no dumps, the milliseconds of the four member functions on stderr (tools/rsets_rate.py)
static double now_ms() { return chrono::duration<double, milli>(chrono::steady_clock::now().time_since_epoch()).count(); }
static void dump(const string &dir, const string &p, DividedPCLReadsSets *s, size_t L) {
    if (timing) return;
    PackedConstantLengthReadsSet *set[3] = {s->getHqReadsSet(), s->getLqReadsSet(), s->getNReadsSet()};
    const char *name[3] = {"hq", "lq", "n"};
    for (int k = 0; k < 3; k++) {
        if (!set[k]) continue;
        const size_t per = set[k]->getReadsSetProperties()->symbolsCount == 4 ? 4 : 3, rb = (L + per - 1) / per, cnt = set[k]->readsCount();
        wr(dir + "/" + p + name[k], cnt ? (const void *) set[k]->getPackedRead(0) : (const void *) "", cnt * rb);
    }
    vector<uint_reads_cnt_max> &lq = s->getLqReadsIndexesMapping()->getMappingVector();
    wr(dir + "/" + p + "lq_map", lq.data(), lq.size() * sizeof(uint_reads_cnt_max));
    if (s->getNReadsIndexesMapping()) {
        vector<uint_reads_cnt_max> &nm = s->getNReadsIndexesMapping()->getMappingVector();
        wr(dir + "/" + p + "n_map", nm.data(), nm.size() * sizeof(uint_reads_cnt_max));
    }
}
int main(int argc, char **argv) {
    const string dir = argv[1];
    const size_t L = atoi(argv[2]);
    const bool separate_n = atoi(argv[3]);
    timing = argc > 5 && string(argv[5]) == "time";
    Records it(rd(dir + "/reads"), rd(dir + "/quals"), L);
    DividedPCLReadsSets *s = pgrc_ref_divide_quality_original(&it, (uint_read_len_max) L, atof(argv[4]), true, separate_n, false);
    dump(dir, "b_", s, L);
    const string f = rd(dir + "/is_hq"), g = rd(dir + "/is_mapped");
    if (f.size() != s->getHqReadsSet()->readsCount()) { cerr << "is_hq: one flag per HQ read" << endl; return 2; }
    vector<bool> is_hq(f.size()), is_mapped(g.size());
    for (size_t i = 0; i < f.size(); i++) is_hq[i] = f[i] != 0;
    for (size_t i = 0; i < g.size(); i++) is_mapped[i] = g[i] != 0;
    const double t0 = now_ms();
    s->moveLqReadsFromHqReadsSetsToLqReadsSets(is_hq);
    const double t1 = now_ms();
    dump(dir, "m_", s, L);
    const double t2 = now_ms();
    IndexesMapping *hm = s->generateHqReadsIndexesMapping();
    const double t3 = now_ms();
    vector<uint_reads_cnt_max> hq_map;
    for (uint_reads_cnt_max i = 0; i <= hm->getMappedReadsCount(); i++) hq_map.push_back(hm->getReadOriginalIndex(i));
    wr(dir + "/hq_mapping", hq_map.data(), hq_map.size() * sizeof(uint_reads_cnt_max));
    const uint_reads_cnt_max n_beg = s->getLqReadsSet()->readsCount();
    if (g.size() != n_beg + (separate_n ? s->getNReadsSet()->readsCount() : 0)) { cerr << "is_mapped: one flag per LQ and N read" << endl; return 3; }
    const double t4 = now_ms();
    s->removeReadsFromLqReadsSet(is_mapped);                        // pgrc-encoder.cpp:367-372
    const double t5 = now_ms();
    if (separate_n) s->removeReadsFromNReadsSet(is_mapped, n_beg);
    const double t6 = now_ms();
    dump(dir, "r_", s, L);
    if (timing) cerr << "ms " << t1 - t0 << " " << t3 - t2 << " " << t5 - t4 << " " << t6 - t5 << endl;
    return 0;
}
"""


def build_driver(tmp):
    src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fopenmp", "-I" + REF, src, "-o", exe, "-L" + refdir, "-lpgrc_ref", "-Wl,-rpath," + refdir], check=True)
    return exe


def records(rng, plan, L, separate_n):
    """FASTQ records that the reference divides as planned"""
    n = plan.size
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))].copy()
    quals = np.full((n, L), ord("I"), np.uint8)
    quals[plan == LQ, int(L * (1 - ERROR_LIMIT))] = ord("#")
    if separate_n:
        rows = np.flatnonzero(plan == N)
    else:                                   # without an N set an N is a symbol like any other: in reads of every set
        rows = np.flatnonzero(rng.random(n) < 0.2)
    if rows.size:
        reads[rows, rng.integers(0, L, size=rows.size)] = ord("N")
    return reads, quals


def plan_of(kind, rng, n, separate_n):
    third = [N] if separate_n else [LQ]
    if kind == "single":
        return np.array([HQ], np.uint8)
    body = rng.choice(np.array([HQ, MOVED, LQ] + third, np.uint8), size=n, p=[0.4, 0.25, 0.2, 0.15])
    if kind == "mixed":         # a moved read below the first old LQ index, old LQ entries below the smallest index that stays HQ, N between
        body = np.concatenate([np.array([MOVED, LQ, LQ] + third + [HQ], np.uint8), body, np.array([HQ, LQ] + third + [MOVED], np.uint8)])
    if kind == "earlyend":      # old LQ entries below every HQ index: the reference's backward walk ends before it reaches them
        body = np.concatenate([np.array([LQ, LQ] + third + [LQ, MOVED, HQ], np.uint8), body])
    if kind == "noflag":
        body[body == HQ] = MOVED
    if kind == "allflags":
        body[body == MOVED] = HQ
    if kind == "lqempty":
        body[body == LQ] = HQ
    return body


def ends_mixed(part):
    """kept and removed rows at both ends"""
    return part.size >= 4 and part[:2].any() and not part[:2].all() and part[-2:].any() and not part[-2:].all()


# (name, kind, seed, reads, L, separate N)
CASES = [("L21_sepN_mixed", "mixed", 1, 200, 21, True), ("L150_sepN_mixed", "mixed", 2, 200, 150, True),
         ("L21_plain_mixed", "mixed", 3, 200, 21, False), ("L150_plain_mixed", "mixed", 4, 150, 150, False),
         ("L150_sepN_earlyend", "earlyend", 5, 120, 150, True), ("L21_sepN_noflag", "noflag", 6, 90, 21, True),
         ("L21_sepN_allflags", "allflags", 7, 90, 21, True), ("L150_sepN_lqempty", "lqempty", 8, 90, 150, True),
         ("L21_plain_single", "single", 9, 1, 21, False)]


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, kind, seed, n, L, separate_n in CASES:
            rng = np.random.default_rng(seed)
            plan = plan_of(kind, rng, n, separate_n)
            A = plan.size
            reads, quals = records(rng, plan, L, separate_n)
            in_hq = (plan == HQ) | (plan == MOVED)
            is_hq = (plan[in_hq] == HQ).astype(np.uint8)
            n_lq_after, n_n = int(((plan == LQ) | (plan == MOVED)).sum()), int((plan == N).sum())
            if kind == "noflag":
                is_mapped = np.zeros(n_lq_after + n_n, np.uint8)
            elif kind == "allflags":
                is_mapped = np.ones(n_lq_after + n_n, np.uint8)
            else:
                is_mapped = (rng.random(n_lq_after + n_n) < 0.5).astype(np.uint8)
                for lo, hi in ((0, n_lq_after), (n_lq_after, n_lq_after + n_n)):
                    if hi - lo >= 4:
                        is_mapped[lo:lo + 2] = [0, 1]
                        is_mapped[hi - 2:hi] = [1, 0]
            for f in os.listdir(tmp):
                if f not in ("driver", "driver.cpp"):
                    os.remove(os.path.join(tmp, f))
            for fname, a in (("reads", reads), ("quals", quals), ("is_hq", is_hq), ("is_mapped", is_mapped)):
                a.tofile(os.path.join(tmp, fname))
            subprocess.run([exe, tmp, str(L), str(int(separate_n)), str(ERROR_LIMIT)], check=True, stdout=subprocess.DEVNULL)
            sym, rb = ru.set_shapes(L, separate_n)
            out = {"L": np.int64(L), "separate_n": np.int64(separate_n), "A": np.int64(A), "is_hq": is_hq, "is_mapped": is_mapped,
                   "hq_mapping": np.fromfile(os.path.join(tmp, "hq_mapping"), dtype=np.uint32)}
            for p in ("b_", "m_", "r_"):
                for k, s in enumerate(("hq", "lq", "n")):
                    if rb[k]:
                        out[p + s] = np.fromfile(os.path.join(tmp, p + s), dtype=np.uint8).reshape(-1, rb[k])
                out[p + "lq_map"] = np.fromfile(os.path.join(tmp, p + "lq_map"), dtype=np.uint32)
                if separate_n:
                    out[p + "n_map"] = np.fromfile(os.path.join(tmp, p + "n_map"), dtype=np.uint32)
            path = os.path.join(HERE, f"rsets_{name}.npz")
            np.savez_compressed(path, **out)
            fx = ru.load_fixture(os.path.basename(path))
            b, m, r = fx["before"], fx["moved"], fx["removed"]
            # the reference divided as planned; what the case stands for, from its own output
            assert np.array_equal(b["lq_map"], np.concatenate([np.flatnonzero(plan == LQ), [A]])), name
            assert b["hq"].shape[0] == int(in_hq.sum()) and m["lq"].shape[0] == n_lq_after and m["lq_map"][-1] == A and r["lq_map"][-1] == A, name
            if separate_n:
                assert np.array_equal(b["n_map"], np.concatenate([np.flatnonzero(plan == N), [A]])) and r["n_map"][-1] == A, name
            lq, moved, stays = b["lq_map"][:-1], np.flatnonzero(plan == MOVED), np.flatnonzero(plan == HQ)
            if kind == "mixed":
                assert moved.min() < lq.min() and moved.max() > lq.max(), name
                assert (lq < stays.min()).any(), name
                if separate_n:
                    nn = b["n_map"][:-1]
                    assert ((nn > lq.min()) & (nn < stays.min())).any() and ((nn > lq.max()) & (nn < moved.max())).any(), name
                    assert ends_mixed(is_mapped[:n_lq_after]) and ends_mixed(is_mapped[n_lq_after:]), name
                else:
                    assert ends_mixed(is_mapped), name
            if kind == "earlyend":
                assert lq[:2].max() < min(moved.min(), stays.min()), name
            if kind == "noflag":
                assert not is_hq.any() and not is_mapped.any() and m["hq"].shape[0] == 0 and ru.same_state(m, r), name
            if kind == "allflags":
                assert is_hq.all() and is_mapped.all() and ru.same_state(b, m) and r["lq"].shape[0] == 0 and r["n"].shape[0] == 0, name
            if kind == "lqempty":
                assert b["lq"].shape[0] == 0 and m["lq"].shape[0] == moved.size > 0, name
            if kind == "single":
                assert A == 1 and b["hq"].shape[0] == 1, name
            assert os.path.getsize(path) < 64 << 10, name
            print(name, "A", A, "before", [b[k].shape[0] if b[k] is not None else None for k in ("hq", "lq", "n")],
                  "moved", int(moved.size), "kept", [r[k].shape[0] if r[k] is not None else None for k in ("hq", "lq", "n")], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
