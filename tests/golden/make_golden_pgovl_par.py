#!/usr/bin/env python3
"""Golden fixtures of the overlap search under the rule of the parallel generator (PGRC_OVL_RULE_PARALLEL), made by the REAL
reference compiled in the build container (oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, builds a
PackedConstantLengthReadsSet from ASCII reads and, with PgHelpers::numberOfThreads = 1 and again = 8,
  - raises __gnu_parallel::_Settings::sort_minimal_n so that the sort of the reads stays sequential (the parallel sort is
    unstable in a way that depends on the thread count; the order among equal reads is an input of the device);
  - sorts the read numbers 1 .. R as prepareSortedReadsBlocks does (ParallelGreedySwipingPackedOverlapPseudoGenomeGenerator.cpp:
    121-124) and records the order;
  - runs init(false) and findOverlappingReads(coef, false) on ParallelGreedySwipingPackedOverlapGeneratorTemplate
    <uint_read_len_min, uint_reads_cnt_std> and dumps nextRead, overlap and the log's numbers;
  - calls getBothSidesOverlappedReads(coef) on a second generator over the same set and dumps the flags.
Both thread counts must give the same bytes, and the chains of equal reads must follow the recorded order.

Fixtures are data only.  The ten settings of make_golden_pgovl.PGOVL_CASES plus an L = 4 and an L = 5 set in each alphabet (every
sweep is one of the last three there).  A set is only kept if neither the reference's own compares (tests/pgovl_par_util.literal)
nor the device's (parallel_form) run past the last row: otherwise its seed moves on by 1000 until they do not.  Asserted:
literal == parallel_form == reference on every fixture; each of the four simplifications misses at least one fixture; every
counter is non-zero over the whole set.  The counts go to manifest_pgovl_par.json.

    python tests/golden/make_golden_pgovl_par.py      # needs the reference tree (run `make -C oracle ref` first)
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
sys.path.insert(0, HERE)

import pgovl_par_util as pp  # noqa: E402
import pgovl_util as po  # noqa: E402
from make_golden_pgovl import MAX_BYTES, PGOVL_CASES, REF, make_codes  # noqa: E402

# (name, kind, seed, R, L, symbols, coef)
PAR_CASES = list(PGOVL_CASES) + [
    ("tail_acgt_L4", "tiny", 321, 160, 4, 4, 1.0),
    ("tail_acgnt_L4", "tiny", 322, 300, 4, 5, 1.0),
    ("tail_acgt_L5", "tiny", 323, 500, 5, 4, 1.0),
    ("tail_acgnt_L5", "tiny", 324, 900, 5, 5, 1.0),
]
SIMPLIFICATIONS = {"no_block_reset": dict(reset=False), "no_quirk": dict(quirk=False), "drop_rule_kept": dict(drop=True),
                   "round_robin_after_tail": dict(concat=False)}
COUNTERS = ("resets_changing", "follower_compares", "glued", "self_conflicts", "would_drop")

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
#include <omp.h>
#include <parallel/algorithm>
#include <parallel/settings.h>
#define protected public
#define private public
#include "pseudogenome/generator/ParallelGreedySwipingPackedOverlapPseudoGenomeGenerator.h"
#undef private
#undef protected
using namespace std;
using namespace PgTools;
using namespace PgIndex;
typedef ParallelGreedySwipingPackedOverlapGeneratorTemplate<uint_read_len_min, uint_reads_cnt_std> Gen;
static void wr(const string &p, const void *d, size_t n) { ofstream f(p, ios::binary); f.write((const char *) d, n); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const int L = atoi(argv[2]), symbols = atoi(argv[3]);
    const double coef = atof(argv[4]);
    const int threads = atoi(argv[5]);
    omp_set_num_threads(threads);
    PgHelpers::numberOfThreads = threads;
    __gnu_parallel::_Settings st = __gnu_parallel::_Settings::get();
    st.sort_minimal_n = ~(__gnu_parallel::_SequenceIndex) 0 >> 1;
    __gnu_parallel::_Settings::set(st);
    ifstream f(dir + "/reads", ios::binary);
    stringstream ss;
    ss << f.rdbuf();
    const string raw = ss.str();
    const size_t R = raw.size() / L;
    PackedConstantLengthReadsSet *set = new PackedConstantLengthReadsSet(L, symbols == 4 ? "ACGT" : "ACGNT", symbols);
    set->reserve(R);
    for (size_t i = 0; i < R; i++) set->addRead(raw.data() + i * L, L);
    const size_t rb = symbols == 4 ? (L + 3) / 4 : (L + 2) / 3;
    wr(dir + "/rows", set->getPackedRead(0), R * rb);
    ostringstream log;                                      // the reference logs to std::cout: its lines are kept instead
    streambuf *const cout_buf = cout.rdbuf(log.rdbuf());
    ParallelGreedySwipingPackedOverlapPseudoGenomeGeneratorFactory factory;
    Gen *gen = dynamic_cast<Gen *>(factory.getGenerator(set, false));
    if (!gen) return 2;
    vector<uint_reads_cnt_std> order;
    for (uint_reads_cnt_std i = 1; i <= R; i++) order.push_back(i);
    auto cmp = [set](uint_reads_cnt_std l, uint_reads_cnt_std r) { return set->comparePackedReads(l - 1, r - 1) < 0; };
    __gnu_parallel::sort(order.begin(), order.end(), cmp);
    wr(dir + "/order", order.data(), R * sizeof(uint_reads_cnt_std));
    gen->init(false);
    gen->findOverlappingReads(coef, false);
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
    src = os.path.join(tmp, "driver_par.cpp")
    exe = os.path.join(tmp, "driver_par")
    with open(src, "w") as f:
        f.write(DRIVER)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fopenmp", "-I" + REF, src, "-o", exe, "-L" + refdir, "-lpgrc_ref",
                    "-Wl,-rpath," + refdir], check=True)
    return exe


def par_codes(kind, seed, R, L, symbols):
    if kind == "tiny":
        return np.random.default_rng(seed).integers(0, symbols, size=(R, L)).astype(np.uint8)
    return make_codes(kind, seed, R, L, symbols)


def reference_run(exe, tmp, reads, L, symbols, coef, threads):
    reads.tofile(os.path.join(tmp, "reads"))
    subprocess.run([exe, tmp, str(L), str(symbols), repr(coef), str(threads)], check=True, stdout=subprocess.DEVNULL)
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


def agrees(res, fx):
    return (np.array_equal(res["next_read"], fx["next_read"]) and np.array_equal(res["overlap"], fx["overlap"].astype(np.uint16))
            and np.array_equal(res["reads_left"], fx["reads_left"]))


def conditions(fx):
    """the manifest's figures: the counters on the fixture's input, and which simplifications miss the fixture"""
    symbols = int(fx["symbols"])
    codes = po.to_codes(fx["reads"], symbols)
    coef = float(fx["coef"])
    lit = pp.literal(codes, fx["sorted_order"], coef, symbols)
    got = pp.parallel_form(codes, fx["sorted_order"], coef, symbols)
    assert agrees(lit, fx), "the literal loops miss the reference"
    assert agrees(got, fx), "the rule misses the reference"
    c = dict(got["counters"], reference_follower_compares=lit["counters"]["follower_compares"],
             reference_past_end_compares=lit["counters"]["past_end_compares"], reads=int(codes.shape[0]), duplicates=int(got["duplicates"]),
             links=int(got["links"]), sweeps=int(got["sweeps"]), tail_sweeps=pp.tail_sweeps(codes.shape[1], coef))
    c["differs_serial_rule"] = int(not agrees(po.literal(codes, fx["sorted_order"], coef, symbols), fx))
    for name, kw in SIMPLIFICATIONS.items():
        c["differs_" + name] = int(not agrees(pp.parallel_form(codes, fx["sorted_order"], coef, symbols, **kw), fx))
    return c


def check_set(manifest):
    for k in COUNTERS:
        assert sum(m[k] for m in manifest.values()) > 0, k
    for name in SIMPLIFICATIONS:
        assert any(m["differs_" + name] for m in manifest.values()), name
    assert all(m["past_end_compares"] == 0 and m["reference_past_end_compares"] == 0 for m in manifest.values())
    assert any(m["differs_serial_rule"] for m in manifest.values())
    assert {m["L"] for m in manifest.values()} >= {4, 5, 12, 33, 40, 150} and {m["coef"] for m in manifest.values()} >= {1.0, 0.5}
    assert {(m["L"], m["symbols"]) for m in manifest.values()} >= {(4, 4), (4, 5), (5, 4), (5, 5)}


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, kind, seed0, R, L, symbols, coef in PAR_CASES:
            for seed in range(seed0, seed0 + 20000, 1000):
                codes = par_codes(kind, seed, R, L, symbols)
                reads = po.ascii_of(codes, symbols)
                fx = reference_run(exe, tmp, reads, L, symbols, coef, 1)
                fx8 = reference_run(exe, tmp, reads, L, symbols, coef, 8)
                assert all(np.array_equal(fx[k], fx8[k]) for k in fx), f"{name}: 1 and 8 threads differ"
                assert po.order_is_sorted(codes, fx["sorted_order"]), name
                # the chains of equal reads follow the recorded order
                o = fx["sorted_order"].astype(np.int64)
                eq = (codes[o[:-1] - 1] == codes[o[1:] - 1]).all(axis=1)
                assert np.array_equal(fx["next_read"][o[:-1][eq]], o[1:][eq]) and (fx["overlap"][o[:-1][eq]] == L).all(), name
                assert fx["reads_left"].size == max(po.iterations(L, coef), 1), name
                assert np.array_equal(fx["flags"], po.both_sides(fx["next_read"], fx["overlap"], L)), name
                c = conditions(fx)
                if c["past_end_compares"] == 0 and c["reference_past_end_compares"] == 0:
                    break
                print(f"{name}: seed {seed} has a compare past the last row, moving on")
            else:
                raise AssertionError(f"{name}: no seed without a compare past the last row")
            path = os.path.join(HERE, f"pgovlpar_{name}.npz")
            np.savez_compressed(path, **fx)
            assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes, the limit is {MAX_BYTES}"
            manifest[name] = dict(c, kind=kind, seed=seed, L=L, symbols=symbols, coef=coef, bytes=os.path.getsize(path))
            print(name, manifest[name])
    check_set(manifest)
    with open(os.path.join(HERE, "manifest_pgovl_par.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
