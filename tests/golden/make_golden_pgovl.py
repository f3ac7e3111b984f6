#!/usr/bin/env python3
"""Golden fixtures of the overlap search (pgrc_ovl_run), made by the REAL reference compiled in the build container
(oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, builds a
PackedConstantLengthReadsSet from ASCII reads and, at one thread,
  - sorts the read numbers 1 .. R by the comparison of the generator's PackedReadsComparator (comparePackedReads(l - 1, r - 1)
    < 0) with __gnu_parallel::sort, the call of initAndFindDuplicates (GreedySwipingPackedOverlapPseudoGenomeGenerator.cpp:
    101-105): the order among equal reads is whatever that sort leaves, so it is recorded and handed to the device as an input;
  - runs init(false) and findOverlappingReads(coef, false) on GreedySwipingPackedOverlapGeneratorTemplate<uint_read_len_min,
    uint_reads_cnt_std> and dumps nextRead and overlap; the "Found <n> duplicates" and "<n> reads left after <m> overlap" lines
    of its log (:135, :149) give the reads-left numbers;
  - calls getBothSidesOverlappedReads(coef) on a second generator over the same set and dumps the flags.

Fixtures are data only: the ASCII reads, the packed rows, the sorted order, nextRead, overlap, the logged numbers, the flags.
Asserted here, from the counters of tests/pgovl_util.parallel_form (which must equal the reference on every case), over the
whole set: at least 20 runs of equal suffixes shared by groups whose order is not the symbol order, 20 round-robin runs, 3 self
conflicts, 20 dropped suffixes, 20 duplicates; and each of the three simplifications of the rule (ties between groups in
symbol order, a group's equal suffixes in one piece, no drop rule) differs from the reference on at least one fixture.  The
counts go to manifest_pgovl.json.

    python tests/golden/make_golden_pgovl.py      # needs the reference tree (run `make -C oracle ref` first)
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pgovl_util as po  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")
MAX_BYTES = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("pgmap_") and f.endswith(".npz"))

# (name, kind, seed, R, L, symbols, coef)
PGOVL_CASES = [
    ("genome_acgt_L40", "genome", 301, 1500, 40, 4, 1.0),
    ("genome_acgnt_L33", "genome", 302, 1200, 33, 5, 0.5),
    ("genome_acgt_L150", "genome", 303, 500, 150, 4, 1.0),
    ("lowcomp_acgt_L12", "periodic", 304, 600, 12, 4, 1.0),
    ("lowcomp_acgnt_L40", "periodic", 305, 500, 40, 5, 0.5),
    ("two_letter_acgt_L33", "two", 306, 900, 33, 4, 1.0),
    ("two_letter_acgnt_L12", "two", 307, 700, 12, 5, 1.0),
    ("mixed_acgnt_L40", "mixed", 308, 900, 40, 5, 1.0),
    ("no_equal_reads", "unique", 309, 800, 40, 4, 1.0),
    ("one_read", "one", 310, 1, 40, 4, 1.0),
]
LIMITS = {"tie_runs_off_symbol_order": 20, "round_robin_runs": 20, "self_conflicts": 3, "dropped": 20, "duplicates": 20}
SIMPLIFICATIONS = {"ties_in_symbol_order": dict(ties="symbol"), "no_round_robin": dict(round_robin=False), "no_drop_rule": dict(drop=False)}

DRIVER = r"""
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include <chrono>
#include <omp.h>
#include <parallel/algorithm>
#define protected public
#define private public
#include "pseudogenome/generator/GreedySwipingPackedOverlapPseudoGenomeGenerator.h"
#undef private
#undef protected
using namespace std;
using namespace PgTools;
using namespace PgIndex;
typedef GreedySwipingPackedOverlapGeneratorTemplate<uint_read_len_min, uint_reads_cnt_std> Gen;
static void wr(const string &p, const void *d, size_t n) { ofstream f(p, ios::binary); f.write((const char *) d, n); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const int L = atoi(argv[2]), symbols = atoi(argv[3]);
    const double coef = atof(argv[4]);
    const bool timing_only = argc > 5;
    omp_set_num_threads(1);
    PgHelpers::numberOfThreads = 1;
    ifstream f(dir + "/reads", ios::binary);
    stringstream ss;
    ss << f.rdbuf();
    const string raw = ss.str();
    const size_t R = raw.size() / L;
    PackedConstantLengthReadsSet *set = new PackedConstantLengthReadsSet(L, symbols == 4 ? "ACGT" : "ACGNT", symbols);
    set->reserve(R);
    for (size_t i = 0; i < R; i++) set->addRead(raw.data() + i * L, L);
    const size_t rb = symbols == 4 ? (L + 3) / 4 : (L + 2) / 3;
    if (!timing_only) wr(dir + "/rows", set->getPackedRead(0), R * rb);
    ostringstream log;                                      // the reference logs to std::cout: its lines are kept instead
    streambuf *const cout_buf = cout.rdbuf(log.rdbuf());
    GreedySwipingPackedOverlapPseudoGenomeGeneratorFactory factory;
    Gen *gen = dynamic_cast<Gen *>(factory.getGenerator(set, false));
    if (!gen) return 2;
    if (!timing_only) {
        vector<uint_reads_cnt_std> order;
        for (uint_reads_cnt_std i = 1; i <= R; i++) order.push_back(i);
        // PackedReadsComparator (GreedySwipingPackedOverlapPseudoGenomeGenerator.h:24-31): compareReads(l, r) < 0
        auto cmp = [set](uint_reads_cnt_std l, uint_reads_cnt_std r) { return set->comparePackedReads(l - 1, r - 1) < 0; };
        __gnu_parallel::sort(order.begin(), order.end(), cmp);
        wr(dir + "/order", order.data(), R * sizeof(uint_reads_cnt_std));
    }
    gen->init(false);
    const auto t0 = chrono::steady_clock::now();
    gen->findOverlappingReads(coef, false);
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    wr(dir + "/ms", &ms, sizeof(ms));
    if (timing_only) {
        cout.rdbuf(cout_buf);
        return 0;
    }
    wr(dir + "/next", gen->nextRead, (R + 1) * sizeof(uint_reads_cnt_std));
    wr(dir + "/ovl", gen->overlap, (R + 1) * sizeof(uint_read_len_min));
    cout.rdbuf(cout_buf);
    const string text = log.str();
    wr(dir + "/log", text.data(), text.size());
    cout.rdbuf(log.rdbuf());
    PseudoGenomeGeneratorBase *gen2 = factory.getGenerator(set, false);
    const vector<bool> hq = gen2->getBothSidesOverlappedReads(coef);
    vector<uint8_t> flags(hq.begin(), hq.end());
    wr(dir + "/flags", flags.data(), flags.size());
    cout.rdbuf(cout_buf);
    return 0;
}
"""


def build_driver(tmp: str) -> str:
    src = os.path.join(tmp, "driver.cpp")
    exe = os.path.join(tmp, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fopenmp", "-I" + REF, src, "-o", exe, "-L" + refdir, "-lpgrc_ref",
                    "-Wl,-rpath," + refdir], check=True)
    return exe


def make_codes(kind, seed, R, L, symbols):
    """the reads of a case as symbol places, uint8 [R, L]"""
    rng = np.random.default_rng(seed)
    if kind == "genome":
        return po.gen_genome(rng, R, L, symbols, coverage=30.0, subst=0.01, dup=0.03)
    if kind == "periodic":
        return po.gen_periodic(rng, R, L, symbols, max_period=4, letters=3)
    if kind == "two":
        return po.gen_genome(rng, R, L, symbols, coverage=12.0, subst=0.02, dup=0.02, letters=2)
    if kind == "mixed":
        return po.gen_mixed(rng, R, L, symbols)
    if kind == "unique":
        reads = np.unique(po.gen_genome(rng, R, L, symbols, coverage=30.0, subst=0.01, dup=0.0), axis=0)
        return reads[rng.permutation(reads.shape[0])]
    return rng.integers(0, symbols, size=(1, L)).astype(np.uint8)


def reference_run(exe, tmp, reads, L, symbols, coef):
    """reads: uint8 [R, L] ASCII -> the fixture"""
    reads.tofile(os.path.join(tmp, "reads"))
    subprocess.run([exe, tmp, str(L), str(symbols), repr(coef)], check=True, stdout=subprocess.DEVNULL)
    R = reads.shape[0]

    def rd(name, dt):
        return np.fromfile(os.path.join(tmp, name), dtype=dt)
    log = open(os.path.join(tmp, "log")).read()
    left = [R - int(re.search(r"Found (\d+) duplicates", log).group(1))]
    left += [int(x) for x in re.findall(r"(\d+) reads left after \d+ overlap", log)]
    out = {"reads": reads, "rows": rd("rows", np.uint8).reshape(R, -1), "sorted_order": rd("order", np.uint32), "next_read": rd("next", np.uint32),
           "overlap": rd("ovl", np.uint8), "reads_left": np.array(left, dtype=np.uint64), "flags": rd("flags", np.uint8),
           "L": np.int64(L), "symbols": np.int64(symbols), "coef": np.float64(coef)}
    assert np.array_equal(out["rows"], po.pack_rows(reads, symbols))
    return out


def reference_ms(exe, tmp, reads, L, symbols, coef):
    """wall time of the reference's serial findOverlappingReads on the set (tools/pgovl_rate.py)"""
    reads.tofile(os.path.join(tmp, "reads"))
    subprocess.run([exe, tmp, str(L), str(symbols), repr(coef), "time"], check=True, stdout=subprocess.DEVNULL)
    return float(np.fromfile(os.path.join(tmp, "ms"), dtype=np.float64)[0])


def conditions(fx):
    """the manifest's figures: the model's counters on the fixture's input, and which simplifications miss the fixture"""
    codes = po.to_codes(fx["reads"], int(fx["symbols"]))
    coef = float(fx["coef"])
    want = {"next_read": fx["next_read"], "overlap": fx["overlap"].astype(np.uint16)}
    got = po.parallel_form(codes, fx["sorted_order"], coef)
    assert np.array_equal(got["next_read"], want["next_read"]) and np.array_equal(got["overlap"], want["overlap"]), "the rule misses the reference"
    c = dict(got["counters"], reads=int(codes.shape[0]), duplicates=int(got["duplicates"]), links=int(got["links"]), sweeps=int(got["sweeps"]),
             equal_reads=int(codes.shape[0] - np.unique(codes, axis=0).shape[0]))
    for name, kw in SIMPLIFICATIONS.items():
        alt = po.parallel_form(codes, fx["sorted_order"], coef, **kw)
        c["differs_" + name] = int(not (np.array_equal(alt["next_read"], want["next_read"]) and np.array_equal(alt["overlap"], want["overlap"])))
    return c


def check_set(manifest):
    for k, lim in LIMITS.items():
        assert sum(m[k] for m in manifest.values()) >= lim, (k, lim)
    for name in SIMPLIFICATIONS:
        assert any(m["differs_" + name] for m in manifest.values()), name
    assert manifest["no_equal_reads"]["equal_reads"] == 0 and manifest["no_equal_reads"]["duplicates"] == 0
    assert manifest["one_read"]["reads"] == 1
    assert {m["L"] for m in manifest.values()} >= {12, 33, 40, 150} and {m["coef"] for m in manifest.values()} >= {1.0, 0.5}
    assert {m["symbols"] for m in manifest.values()} == {4, 5}


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, kind, seed, R, L, symbols, coef in PGOVL_CASES:
            codes = make_codes(kind, seed, R, L, symbols)
            fx = reference_run(exe, tmp, po.ascii_of(codes, symbols), L, symbols, coef)
            assert po.order_is_sorted(codes, fx["sorted_order"]), name
            assert fx["reads_left"].size == max(po.iterations(L, coef), 1), name
            assert np.array_equal(fx["flags"], po.both_sides(fx["next_read"], fx["overlap"], L)), name
            c = conditions(fx)
            path = os.path.join(HERE, f"pgovl_{name}.npz")
            np.savez_compressed(path, **fx)
            assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes, the limit is {MAX_BYTES}"
            manifest[name] = dict(c, kind=kind, seed=seed, L=L, symbols=symbols, coef=coef, bytes=os.path.getsize(path))
            print(name, manifest[name])
    check_set(manifest)
    with open(os.path.join(HERE, "manifest_pgovl.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
