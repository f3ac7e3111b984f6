#!/usr/bin/env python3
"""Golden fixtures of the pseudogenome assembly (pgrc_asm_run), made by the REAL reference compiled in the build container
(oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, builds a
PackedConstantLengthReadsSet from ASCII reads, gets the generator from GreedySwipingPackedOverlapPseudoGenomeGeneratorFactory and
runs, on AbstractOverlapPseudoGenomeGeneratorTemplate<uint_read_len_min, uint_reads_cnt_std>: init(true),
performOverlapping(coef, false) -- nextRead and overlap dumped --, removeCyclesAndPrepareComponents() -- both dumped again,
with headRead --, countPseudoGenomeLength(), countComponents(), countSingles() and
assemblePseudoGenomeTemplate<GeneratedSeparatedPseudoGenome>() -- the sequence, off and orgIdx dumped.  The cycles' count and
the lost symbols are read from the reference's own log line.  With coef = 1 the driver also asserts that a plain
generateSeparatedPseudoGenome() of the same set gives the same sequence, off and orgIdx (with a smaller coef that call would
overlap further, so the set without any overlap is not compared).

Fixtures are data only: the packed rows, nextRead and overlap before and after the cuts, the outputs and the logged numbers.
Asserted here against the reference's own output, for every mixed case: at least 3 cycles; a cycle of two reads or more
whose chain after the cut does not start at the cycle's smallest index (the first read of the cycle that the ascending loops
come to); at least 20 duplicates (overlap = L); a chain of at least 300 reads; at least 10 singles.  The counts go to
manifest_pgasm.json.

    python tests/golden/make_golden_pgasm.py      # needs the reference tree (run `make -C oracle ref` first)
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

import pgasm_util as pa  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")
MAX_BYTES = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("pgmap_") and f.endswith(".npz"))

# (name, mixed, seed, L, symbols, coef)
PGASM_CASES = [
    ("mixed_acgt", True, 71, 40, 4, 1.0),
    ("mixed_acgnt", True, 72, 41, 5, 1.0),
    ("no_overlap", False, 73, 40, 4, 0.026),        # just above 1 / L: no sweep runs, distinct reads stay singles
    ("one_read", False, 74, 40, 4, 1.0),
]
# circular genomes of the mixed cases: (length, step between reads); one is shorter than a read
CIRCLES = [(90, 1), (120, 2), (150, 3), (61, 1), (100, 2), (33, 3)]

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
#define protected public
#include "pseudogenome/generator/GreedySwipingPackedOverlapPseudoGenomeGenerator.h"
#include "pseudogenome/SeparatedPseudoGenome.h"
#undef protected
using namespace std;
using namespace PgTools;
using namespace PgIndex;
typedef AbstractOverlapPseudoGenomeGeneratorTemplate<uint_read_len_min, uint_reads_cnt_std> Gen;
static void wr(const string &p, const void *d, size_t n) { ofstream f(p, ios::binary); f.write((const char *) d, n); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const int L = atoi(argv[2]), symbols = atoi(argv[3]);
    const double coef = atof(argv[4]);
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
    GreedySwipingPackedOverlapPseudoGenomeGeneratorFactory factory;
    Gen *gen = dynamic_cast<Gen *>(factory.getGenerator(set, false));
    if (!gen) return 2;
    gen->init(true);
    gen->performOverlapping(coef, false);
    wr(dir + "/next0", gen->nextRead, (R + 1) * sizeof(uint_reads_cnt_std));
    wr(dir + "/ovl0", gen->overlap, (R + 1) * sizeof(uint_read_len_min));
    gen->removeCyclesAndPrepareComponents();
    wr(dir + "/next1", gen->nextRead, (R + 1) * sizeof(uint_reads_cnt_std));
    wr(dir + "/ovl1", gen->overlap, (R + 1) * sizeof(uint_read_len_min));
    wr(dir + "/head1", gen->headRead, (R + 1) * sizeof(uint_reads_cnt_std));
    gen->pseudoGenomeLength = gen->countPseudoGenomeLength();
    const uint64_t nums[3] = {(uint64_t) gen->pseudoGenomeLength, (uint64_t) gen->countComponents(), (uint64_t) gen->countSingles()};
    wr(dir + "/nums", nums, sizeof(nums));
    GeneratedSeparatedPseudoGenome *pg = gen->assemblePseudoGenomeTemplate<GeneratedSeparatedPseudoGenome>();
    const string seq = pg->getPgSequence();
    const vector<uint_read_len_min> off = pg->getReadsList()->off;
    const vector<uint_reads_cnt_std> org = pg->getReadsList()->orgIdx;
    wr(dir + "/seq", seq.data(), seq.size());
    wr(dir + "/off", off.data(), off.size() * sizeof(off[0]));
    wr(dir + "/org", org.data(), org.size() * sizeof(org[0]));
    cout.rdbuf(cout_buf);
    const string text = log.str();
    wr(dir + "/log", text.data(), text.size());
    if (coef == 1.0) {
        PseudoGenomeGeneratorBase *gen2 = factory.getGenerator(set, false);
        SeparatedPseudoGenome *pg2 = gen2->generateSeparatedPseudoGenome();
        if (pg2->getPgSequence() != seq || pg2->getReadsList()->off != off || pg2->getReadsList()->orgIdx != org) return 3;
    }
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


def make_reads(name, seed, L, symbols):
    """the ASCII reads of a case, uint8 [R, L]"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if name == "one_read":
        return acgt[rng.integers(0, 4, size=(1, L))]
    if name == "no_overlap":
        reads = np.unique(acgt[rng.integers(0, 4, size=(600, L))], axis=0)
        return reads[rng.permutation(reads.shape[0])]
    parts = []
    # reads sampled from a linear random genome (dense: long chains and natural duplicates); with ACGNT a few N's in the genome
    genome = acgt[rng.integers(0, 4, size=4000)]
    if symbols == 5:
        genome[rng.choice(genome.size, size=6, replace=False)] = ord("N")
    pos = rng.integers(0, genome.size - L + 1, size=2400)
    parts.append(genome[pos[:, None] + np.arange(L)[None, :]])
    # circular genomes whose reads step by 1, 2 and 3 all the way round
    for clen, step in CIRCLES:
        circ = acgt[rng.integers(0, 4, size=clen)]
        st = np.arange(0, clen, step)
        parts.append(circ[(st[:, None] + np.arange(L)[None, :]) % clen])
    # planted duplicates
    lin = parts[0]
    parts.append(lin[rng.integers(0, lin.shape[0], size=30)])
    # reads of their own: A, random symbols, C -- what the sweep down to an overlap of 1 leaves of them are the singles
    own = acgt[rng.integers(0, 4, size=(60, L))]
    own[:, 0] = ord("A")
    own[:, -1] = ord("C")
    parts.append(own)
    reads = np.concatenate(parts)
    return reads[rng.permutation(reads.shape[0])]


def reference_run(exe, tmp, reads, L, symbols, coef):
    reads.tofile(os.path.join(tmp, "reads"))
    subprocess.run([exe, tmp, str(L), str(symbols), repr(coef)], check=True, stdout=subprocess.DEVNULL)
    R = reads.shape[0]

    def rd(name, dt):
        return np.fromfile(os.path.join(tmp, name), dtype=dt)
    log = open(os.path.join(tmp, "log")).read()
    m = re.search(r"Removed (\d+) cycles \(lost (\d+) symbols\)", log)
    nums = rd("nums", np.uint64)
    out = {"rows": rd("rows", np.uint8).reshape(R, -1), "next_read": rd("next0", np.uint32), "overlap": rd("ovl0", np.uint8),
           "next_read_cut": rd("next1", np.uint32), "overlap_cut": rd("ovl1", np.uint8), "head_read": rd("head1", np.uint32),
           "text": rd("seq", np.uint8), "off": rd("off", np.uint8).astype(np.uint16), "org_idx": rd("org", np.uint32),
           "pg_len": np.uint64(nums[0]), "components": np.uint64(nums[1]), "singles": np.uint64(nums[2]),
           "cycles": np.uint64(m.group(1)), "overlap_lost": np.uint64(m.group(2)),
           "L": np.int64(L), "symbols": np.int64(symbols), "coef": np.float64(coef)}
    assert np.array_equal(out["rows"], pa.pack_rows(reads, symbols))
    return out


def conditions(fx):
    """the manifest's figures, from the reference's output alone"""
    nx0, nx1, ov0, head = fx["next_read"], fx["next_read_cut"], fx["overlap"], fx["head_read"]
    L = int(fx["L"])
    cuts = np.flatnonzero((nx0 != 0) & (nx1 == 0))
    off_head = 0          # cycles of two reads or more whose chain after the cut does not start at the cycle's smallest index
    largest = 0           # cuts at the largest index of their cycle
    for m in cuts:
        members, k = [int(m)], int(nx0[m])
        while k != m:
            members.append(k)
            k = int(nx0[k])
        largest += int(m == max(members))
        off_head += int(len(members) >= 2 and int(nx0[m]) != min(members))
    longest, k = 0, 0
    for h in np.flatnonzero(head[1:] == 0) + 1:
        n, k = 0, int(h)
        while k:
            n += 1
            k = int(nx1[k])
        longest = max(longest, n)
    return {"reads": int(nx0.size - 1), "cycles": int(fx["cycles"]), "cuts": int(cuts.size), "cuts_at_largest": largest, "cycles_off_head": off_head,
            "duplicates": int(((ov0[1:] == L) & (nx0[1:] != 0)).sum()), "longest_chain": longest, "singles": int(fx["singles"]),
            "components": int(fx["components"]), "overlap_lost": int(fx["overlap_lost"]), "pg_len": int(fx["pg_len"]),
            "reads_with_n": int((pa.unpack_rows(fx["rows"], L, int(fx["symbols"])) == ord("N")).any(axis=1).sum())}


def check_mixed(name, c):
    assert c["cycles"] >= 3, f"{name}: {c}"
    assert c["cycles_off_head"] >= 1, f"{name}: {c}"
    assert c["duplicates"] >= 20, f"{name}: {c}"
    assert c["longest_chain"] >= 300, f"{name}: {c}"
    assert c["singles"] >= 10, f"{name}: {c}"


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, mixed, seed, L, symbols, coef in PGASM_CASES:
            reads = make_reads(name, seed, L, symbols)
            fx = reference_run(exe, tmp, reads, L, symbols, coef)
            c = conditions(fx)
            assert c["cuts"] == c["cycles"] == c["cuts_at_largest"], f"{name}: {c}"
            if mixed:
                check_mixed(name, c)
                if symbols == 5:
                    assert c["reads_with_n"] >= 3 and L % 3, f"{name}: {c}"
            if name == "no_overlap":
                assert c["singles"] == c["reads"] and c["pg_len"] == c["reads"] * L, f"{name}: {c}"
            if name == "one_read":
                assert c["reads"] == 1 and c["pg_len"] == L, f"{name}: {c}"
            path = os.path.join(HERE, f"pgasm_{name}.npz")
            np.savez_compressed(path, **fx)
            assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes, the limit is {MAX_BYTES}"
            manifest[name] = dict(c, mixed=mixed, seed=seed, L=L, symbols=symbols, coef=coef, bytes=os.path.getsize(path))
            print(name, manifest[name])
    with open(os.path.join(HERE, "manifest_pgasm.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
