#!/usr/bin/env python3
"""Golden fixtures of the pair-position coding of the order-preserving paired mode (pgrc_pairpos_encode / _decode,
pgrc_decode_set_order_pair_streams), made by the REAL reference compiled in the build container
(oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, calls
SeparatedPseudoGenomePersistence::compressReadsPgPositions<uint_pg_len_std / _max> into a string stream, takes the raw
streams back with readCompressedCollectiveParallel, and runs decompressReadsPgPositions on the same bytes (version 1.3,
not singleReadsMode).  Fixtures are data only: the generator parameters (tests/pairpos_util.make_positions), the input
positions (interleaved), the eight raw streams and the decoded array (file-major, in the position width).  Every mixed
case must hold at least 50 pairs of every kind -- near, delta, setting full, keeping full -- and 50 ties; the counts go
to manifest_pairpos.json.

    python tests/golden/make_golden_pairpos.py      # needs the reference tree (run `make -C oracle ref` first)
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pairpos_util as pp  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")
MAX_BYTES = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("pgmap_") and f.endswith(".npz"))

# (name, mixed, seed, pairs, W, make_positions knobs)
PAIRPOS_CASES = [
    ("w4_mixed", True, 51, 2400, 4, dict(near=0.35, jump=0.22, ret=0.08, tie=0.06, special=0.03)),
    ("w8_above_4g", True, 52, 2000, 8, dict(near=0.35, jump=0.22, ret=0.08, tie=0.06, special=0.03, hi=True)),
    ("all_near", False, 53, 2400, 4, dict(near=1.0, tie=0.02, special=0.05)),
    ("all_far", False, 54, 2400, 4, dict(near=0.0, jump=0.25, ret=0.08, tie=0.02, special=0.03)),
    ("ties_boundaries", True, 55, 2400, 4, dict(near=0.3, jump=0.2, ret=0.1, tie=0.4, special=0.25)),
    ("w8_small_positions", True, 56, 2000, 8, dict(near=0.35, jump=0.22, ret=0.08, tie=0.06, special=0.03, hi=False)),
]

DRIVER = r"""
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "pseudogenome/persistence/SeparatedPseudoGenomePersistence.h"
#include "coders/CodersLib.h"
#include "pgrc/pgrc-params.h"
using namespace std;
using namespace PgTools;
static void wr(const string &p, const char *d, size_t n) { ofstream f(p, ios::binary); f.write(d, n); }
template <typename uint_pg_len>
static int run(const string &dir, const vector<uint_pg_len_max> &org, uint_pg_len_max joinedLen) {
    ostringstream out;
    SeparatedPseudoGenomePersistence::compressReadsPgPositions<uint_pg_len>(out, org, joinedLen, CODER_LEVEL_NORMAL, false, true);
    const string bytes = out.str();
    {
        istringstream in(bytes);
        string s[8];
        vector<string *> dest;
        for (int k = 0; k < 8; k++) dest.push_back(&s[k]);
        readCompressedCollectiveParallel(in, dest);
        for (int k = 0; k < 8; k++) wr(dir + "/stream" + to_string(k), s[k].data(), s[k].size());
    }
    {
        istringstream in(bytes);
        PgRCParams params;
        params.readsTotalCount = org.size();
        params.singleReadsMode = false;
        params.pgrcVersionMajor = 1;
        params.pgrcVersionMinor = 3;
        vector<uint_pg_len> pgPos;
        SeparatedPseudoGenomePersistence::decompressReadsPgPositions<uint_pg_len>(in, pgPos, &params);
        wr(dir + "/decoded", (const char *) pgPos.data(), pgPos.size() * sizeof(uint_pg_len));
    }
    return 0;
}
int main(int argc, char **argv) {
    const string dir = argv[1];
    const int W = atoi(argv[2]);
    ifstream f(dir + "/org", ios::binary);
    stringstream ss;
    ss << f.rdbuf();
    const string raw = ss.str();
    vector<uint_pg_len_max> org(raw.size() / 8);
    memcpy(org.data(), raw.data(), org.size() * 8);
    uint_pg_len_max top = 0;
    for (auto v : org) top = max(top, v);
    return W == 8 ? run<uint_pg_len_max>(dir, org, top + 1) : run<uint_pg_len_std>(dir, org, top + 1);
}
"""

STREAM_DTYPES = (None, np.uint8, np.uint8, np.uint16, np.uint8, np.uint8, np.int16, None)


def build_driver(tmp: str) -> str:
    src = os.path.join(tmp, "driver.cpp")
    exe = os.path.join(tmp, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-fopenmp", "-I" + REF, src, "-o", exe, "-L" + refdir, "-lpgrc_ref",
                    "-Wl,-rpath," + refdir], check=True)
    return exe


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, mixed, seed, pairs, W, knobs in PAIRPOS_CASES:
            org = pp.make_positions(seed, pairs, W, **knobs)
            org.tofile(os.path.join(tmp, "org"))
            subprocess.run([exe, tmp, str(W)], check=True, stdout=subprocess.DEVNULL)
            pdt = pp.pos_dtype(W)
            out = {"seed": np.int64(seed), "pairs": np.int64(pairs), "pos_width": np.int64(W),
                   "knobs": np.frombuffer(json.dumps(knobs, sort_keys=True).encode(), dtype=np.uint8), "org": org}
            st = {"n_total": 2 * pairs, "pos_width": W}
            for k, (sname, dt) in enumerate(zip(pp.STREAMS, STREAM_DTYPES)):
                st[sname] = out[sname] = np.fromfile(os.path.join(tmp, f"stream{k}"), dtype=dt or pdt)
            out["decoded"] = np.fromfile(os.path.join(tmp, "decoded"), dtype=pdt)
            assert np.array_equal(out["decoded"].astype(np.uint64), pp.file_major(org)), f"{name}: the reference's round trip differs from the input"
            counts = dict(pp.kinds(st), ties=pp.ties(org))
            if mixed:
                assert min(counts.values()) >= 50, f"{name}: a kind of pair is missing: {counts}"
            path = os.path.join(HERE, f"pairpos_{name}.npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes, the limit is {MAX_BYTES}"
            manifest[name] = dict(counts, pairs=pairs, pos_width=W, mixed=mixed, bytes=os.path.getsize(path),
                                  above_4g=int((org >> np.uint64(32) != 0).sum()))
            print(name, manifest[name])
    with open(os.path.join(HERE, "manifest_pairpos.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
