#!/usr/bin/env python3
"""Golden fixtures of the pair-order coding of the paired mode that does not preserve the order (pgrc_pairorder_encode),
made by the REAL reference compiled in the build container (oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, calls
SeparatedPseudoGenomePersistence::compressReadsOrder into a string stream, takes the raw streams back with
readCompressedCollectiveParallel (readCompressed for the single-file form), and runs decompressReadsOrder on the same
bytes.  Fixtures are data only: the generator parameters (tests/pairorder_util.make_order), the order `org`, the raw
streams of the form and the decoded rlIdxOrder.  Asserted here against the reference's own streams: every mixed case holds
at least 50 pairs of every kind -- near, delta, setting full, keeping full --, both parities of the base's file flag in
the near and in the far stream, and rel = 255 and 256 and deltas of 127 and -128 at least once each; the counts go to
manifest_pairorder.json.  (The single-file form writes rev alone: its counts are those of the reference's streams for the
same order in the COMPLETE form.)

    python tests/golden/make_golden_pairorder.py      # needs the reference tree (run `make -C oracle ref` first)
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

import pairorder_util as po  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")
MAX_BYTES = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("pgmap_") and f.endswith(".npz"))

MIXED = dict(near=0.3, jump=0.3, ret=0.15, special=0.06, drift=150, span=1 << 12)
# (name, mixed, seed, pairs, form, make_order knobs)
PAIRORDER_CASES = [
    ("mixed_ignore", True, 61, 2400, po.IGNORE, MIXED),
    ("mixed_file_flags", True, 62, 2400, po.FILE_FLAGS, MIXED),
    ("mixed_complete", True, 63, 2400, po.COMPLETE, MIXED),
    ("mixed_complete_single_file", True, 64, 2400, po.COMPLETE_SINGLE_FILE, MIXED),
    ("all_near", False, 65, 2400, po.FILE_FLAGS, dict(near=1.0, special=0.0)),
    ("all_far", False, 66, 2400, po.FILE_FLAGS, dict(near=0.0, jump=0.2, ret=0.1, special=0.0, drift=100, span=1 << 11, halves=True)),
    ("boundaries", True, 67, 2400, po.COMPLETE, dict(near=0.25, jump=0.2, ret=0.1, special=0.3, drift=250, span=1 << 11)),
    ("one_pair", False, 68, 1, po.FILE_FLAGS, dict()),
]

DRIVER = r"""
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "pseudogenome/persistence/SeparatedPseudoGenomePersistence.h"
#include "coders/CodersLib.h"
using namespace std;
using namespace PgTools;
static void wr(const string &p, const char *d, size_t n) { ofstream f(p, ios::binary); f.write(d, n); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const bool complete = atoi(argv[2]), ignore = atoi(argv[3]), single = atoi(argv[4]);
    ifstream f(dir + "/org", ios::binary);
    stringstream ss;
    ss << f.rdbuf();
    const string raw = ss.str();
    vector<uint_reads_cnt_std> org(raw.size() / sizeof(uint_reads_cnt_std));
    memcpy(org.data(), raw.data(), org.size() * sizeof(uint_reads_cnt_std));
    ostringstream out;
    SeparatedPseudoGenomePersistence::compressReadsOrder(out, org, CODER_LEVEL_NORMAL, complete, ignore, single);
    const string bytes = out.str();
    {
        istringstream in(bytes);
        if (complete && single) {
            string s;
            readCompressed(in, s);
            wr(dir + "/stream0", s.data(), s.size());
        } else {
            const int ns = 5 + (complete ? 1 : (ignore ? 0 : 2));
            string s[7];
            vector<string *> dest;
            for (int k = 0; k < ns; k++) dest.push_back(&s[k]);
            readCompressedCollectiveParallel(in, dest);
            for (int k = 0; k < ns; k++) wr(dir + "/stream" + to_string(k), s[k].data(), s[k].size());
        }
    }
    {
        istringstream in(bytes);
        vector<uint_reads_cnt_std> order;
        SeparatedPseudoGenomePersistence::decompressReadsOrder(in, order, complete, ignore, single);
        wr(dir + "/decoded", (const char *) order.data(), order.size() * sizeof(uint_reads_cnt_std));
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


def reference_streams(exe, tmp, org, form):
    """-> (the reference's streams of `org` in `form`, its decoded rlIdxOrder)"""
    org.tofile(os.path.join(tmp, "org"))
    subprocess.run([exe, tmp] + [str(int(x)) for x in po.FORM_ARGS[form]], check=True, stdout=subprocess.DEVNULL)
    st = {"n_total": org.size, "form": form}
    for k, (name, dt) in enumerate(po.stream_types(form)):
        st[name] = np.fromfile(os.path.join(tmp, f"stream{k}"), dtype=dt)
    return st, np.fromfile(os.path.join(tmp, "decoded"), dtype=np.uint32)


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, mixed, seed, pairs, form, knobs in PAIRORDER_CASES:
            org = po.make_order(seed, pairs, **knobs)
            st, decoded = reference_streams(exe, tmp, org, form)
            out = {"seed": np.int64(seed), "pairs": np.int64(pairs), "form": np.int64(form),
                   "knobs": np.frombuffer(json.dumps(knobs, sort_keys=True).encode(), dtype=np.uint8), "org": org, "decoded": decoded}
            for sname, _ in po.stream_types(form):
                out[sname] = st[sname]
            assert decoded.size == 2 * pairs
            # the kinds, from the reference's streams (of the COMPLETE form where this one codes no pair)
            coded = st if form != po.COMPLETE_SINGLE_FILE else reference_streams(exe, tmp, org, po.COMPLETE)[0]
            counts = dict(po.kinds(coded), **po.boundaries(coded))
            if form == po.FILE_FLAGS:
                for sname in ("off_base_file_flag", "nonoff_base_file_flag"):
                    counts[sname + "_ones"] = int((st[sname] == 1).sum())
                    counts[sname + "_zeros"] = int((st[sname] == 0).sum())
            if mixed:
                assert min(counts[k] for k in ("near", "delta", "full_set", "full_keep")) >= 50, f"{name}: a kind of pair is missing: {counts}"
                assert min(counts[k] for k in ("rel_255", "rel_256", "delta_127", "delta_m128")) >= 1, f"{name}: a boundary value is missing: {counts}"
                if form == po.FILE_FLAGS:
                    assert min(v for k, v in counts.items() if k.endswith(("_ones", "_zeros"))) >= 1, f"{name}: a file-flag parity is missing: {counts}"
            if name == "all_near":
                assert counts["near"] == pairs, counts
            if name == "all_far":
                assert counts["near"] == 0, counts
            path = os.path.join(HERE, f"pairorder_{name}.npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes, the limit is {MAX_BYTES}"
            manifest[name] = dict(counts, pairs=pairs, form=form, mixed=mixed, bytes=os.path.getsize(path))
            print(name, manifest[name])
    with open(os.path.join(HERE, "manifest_pairorder.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
