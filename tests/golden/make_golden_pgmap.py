#!/usr/bin/env python3
"""Golden fixtures of the Pg-vs-Pg marking and its inverse (row f2 and pgrc_decode_set_mapped_text), made by the REAL
reference compiled in the build container (oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, maps the
three texts as SimplePgMatcher::matchPgsInPg does (markAndRemoveExactMatches for LQ, N, then HQ against itself) and
restores them with SimplePgMatcher::restoreMatchedPg.  The raw matches the marking starts from come from the same
reference's CopMEMMatcher::matchTexts (tests/oracle.py ref_mem_match).  Fixtures are data only: the generator parameters
(texts are re-derived by tests/pgmap_util.make_texts; their digests are stored), the raw matches, the mapped bytes and
the streams.

    python tests/golden/make_golden_pgmap.py        # needs the reference tree (run `make -C oracle ref` first)
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as orc  # noqa: E402
import pgmap_util as pu  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")

# (name, seed, G, G_lq, G_n, nrep, chains, chain_depth, low_complexity, target_len)
PGMAP_CASES = [
    ("hq_lq_n", 31, 150000, 50000, 20000, 40, 0, 0, False, 45),
    ("empty_n", 32, 120000, 40000, 0, 40, 0, 0, False, 45),
    ("short_hq", 33, 30, 5000, 3000, 0, 0, 0, False, 45),
    ("low_complexity", 34, 120000, 30000, 10000, 30, 0, 0, True, 36),
    ("rc_chains", 35, 200000, 30000, 8000, 10, 6, 5, False, 45),
]

DRIVER = r"""
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "matching/SimplePgMatcher.h"
using namespace std;
// oracle/ref_harness.cpp: runs CopMEMMatcher::matchTexts; it sets the library's PgHelpers::numberOfThreads and the
// OpenMP threads first (the reference's multi-threaded matcher picks among equal sources in no fixed order)
extern "C" int pgrc_ref_mem_match(const char *, uint64_t, const char *, uint64_t, int, int, uint32_t, uint32_t, uint32_t, int,
                                  uint64_t **, uint64_t *);
extern "C" void pgrc_ref_free(void *);
static string rd(const string &p) { ifstream f(p, ios::binary); stringstream s; s << f.rdbuf(); return s.str(); }
static void wr(const string &p, const string &s) { ofstream f(p, ios::binary); f.write(s.data(), s.size()); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const uint32_t target = (uint32_t) atoi(argv[2]);
    {   // one thread from here on, as ref_mem_match(threads=1) finds the raw matches
        uint64_t *o = nullptr, c = 0;
        const std::string t(64, 'A');
        pgrc_ref_mem_match(t.data(), t.size(), t.data(), t.size(), 0, 0, 32, UINT32_MAX, 32, 1, &o, &c);
        pgrc_ref_free(o);
    }
    string hq = rd(dir + "/hq"), lq = rd(dir + "/lq"), n = rd(dir + "/n");
    const uint64_t orgHq = hq.size();
    string off[3], len[3];
    {
        PgTools::SimplePgMatcher m(hq, target);
        m.markAndRemoveExactMatches(false, lq, off[1], len[1], true);
        m.markAndRemoveExactMatches(false, n, off[2], len[2], true);
        m.markAndRemoveExactMatches(true, hq, off[0], len[0], true);
    }
    const string *mp[3] = {&hq, &lq, &n};
    for (int p = 0; p < 3; p++) {
        wr(dir + "/mapped" + to_string(p), *mp[p]);
        wr(dir + "/off" + to_string(p), off[p]);
        wr(dir + "/len" + to_string(p), len[p]);
    }
    string rhq, rlq, rn;
    istringstream o, l;
    o.str(off[0]); l.str(len[0]);
    rhq = PgTools::SimplePgMatcher::restoreMatchedPg(rhq, orgHq, hq, o, l, true, false, true);
    o.clear(); l.clear(); o.str(off[1]); l.str(len[1]);
    rlq = PgTools::SimplePgMatcher::restoreMatchedPg(rhq, orgHq, lq, o, l, true, false);
    if (!n.empty()) { o.clear(); l.clear(); o.str(off[2]); l.str(len[2]);
        rn = PgTools::SimplePgMatcher::restoreMatchedPg(rhq, orgHq, n, o, l, true, false); }
    wr(dir + "/restored0", rhq); wr(dir + "/restored1", rlq); wr(dir + "/restored2", rn);
    return 0;
}
"""


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()[:16]


def build_driver(tmp: str) -> str:
    src = os.path.join(tmp, "driver.cpp")
    exe = os.path.join(tmp, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-I" + REF, src, "-o", exe, "-L" + refdir, "-lpgrc_ref",
                    "-Wl,-rpath," + refdir], check=True)
    return exe


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, seed, G, Gl, Gn, nrep, chains, depth, lowc, tl in PGMAP_CASES:
            hq, lq, nn = pu.make_texts(seed, G, Gl, Gn, nrep=nrep, chains=chains, chain_depth=depth, low_complexity=lowc)
            for fn, t in (("hq", hq), ("lq", lq), ("n", nn)):
                t.tofile(os.path.join(tmp, fn))
            subprocess.run([exe, tmp, str(tl)], check=True, stdout=subprocess.DEVNULL)
            rd = lambda fn: np.fromfile(os.path.join(tmp, fn), dtype=np.uint8)  # noqa: E731
            out = {"params": np.array([seed, G, Gl, Gn, nrep, chains, depth, int(lowc), tl], dtype=np.int64)}
            for p, t in enumerate((hq, lq, nn)):
                out[f"digest{p}"] = np.frombuffer(digest(t).encode(), dtype=np.uint8)
                for k in ("mapped", "off", "len"):
                    out[f"{k}{p}"] = rd(f"{k}{p}")
                restored = rd(f"restored{p}")
                assert np.array_equal(restored, t), f"{name}: the reference's restore of part {p} differs from the text"
            # the raw matches each markAndRemoveExactMatches call started from (LQ, N against HQ; HQ against itself)
            for p, (dest, dis) in enumerate(((hq, True), (lq, False), (nn, False))):
                if hq.size >= tl and dest.size:
                    m = orc.ref_mem_match(hq, pu.revcomp_np(dest), dis, True, tl, threads=1)
                else:
                    m = np.zeros((0, 3), np.uint64)
                out[f"matches{p}"] = m
            np.savez_compressed(os.path.join(HERE, f"pgmap_{name}.npz"), **out)
            manifest[name] = {"marks": [int((out[f"mapped{p}"] == pu.MATCH_MARK).sum()) for p in range(3)],
                              "mapped_bytes": [int(out[f"mapped{p}"].size) for p in range(3)],
                              "text_bytes": [int(t.size) for t in (hq, lq, nn)]}
            print(name, manifest[name])
    with open(os.path.join(HERE, "manifest_pgmap.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
