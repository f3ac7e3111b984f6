#!/usr/bin/env python3
"""Golden fixtures of the archive form of a reads list's mismatch streams (pgrc_list_archive_encode,
pgrc_decode_add_list_archive), made by the REAL reference compiled in the build container (oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, feeds a
SeparatedPseudoGenomeOutputBuilder with writeReadEntry, calls compressedBuild into a string stream, takes the raw streams back
with the reference's readCompressed (the archive is a plain sequence of such streams after the five bytes of the symbol
order) and runs ExtendedReadsListWithConstantAccessOption::loadConstantAccessExtendedReadsList on the same bytes.  Fixtures
are data only: the inputs (counts, context codes, forward offsets), the reference's raw streams and its loaded misCnt,
misSymCode and forward misOff.  The properties every case stands for are asserted here against the reference's own streams
and go to manifest_listarchive.json.

    python tests/golden/make_golden_listarchive.py      # needs the reference tree (run `make -C oracle ref` first)
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

import listarchive_util as la  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")
MAX_BYTES = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith("pgmap_") and f.endswith(".npz"))

# (name, seed, entries, L, fast, make_list knobs)
CASES = [
    ("mixed", 71, 3000, 150, False, dict(zero=0.6, counts=(1, 2, 3, 5, 6), weights=(8, 5, 3, 2, 1), skew=(5, 3, 8, 2, 1))),
    ("ties", 72, 1500, 150, False, dict(zero=0.5, counts=(1, 2, 3), skew=(0, 1, 0, 1, 0))),
    ("no_mismatches", 73, 700, 150, False, dict(zero=1.0)),
    ("fast", 74, 1500, 150, True, dict(zero=0.5, counts=(1, 2, 3, 4), skew=(1, 2, 3, 4, 1))),
    ("max_one", 75, 1500, 150, False, dict(zero=0.6, counts=(1,), skew=(4, 3, 2, 1, 1))),
    ("wide", 76, 400, 255, False, dict(zero=0.5, counts=(1, 2, 7, 253, 254), weights=(6, 4, 2, 1, 1), skew=(2, 5, 1, 4, 3))),
    ("one_entry", 77, 1, 150, False, dict(zero=0.0, counts=(2,), skew=(1, 1, 1, 1, 1))),
]

DRIVER = r"""
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "pseudogenome/persistence/SeparatedPseudoGenomePersistence.h"
#include "pseudogenome/readslist/SeparatedExtendedReadsList.h"
#include "pseudogenome/SeparatedPseudoGenome.h"
#include "pgrc/pgrc-params.h"
#include "coders/CodersLib.h"
using namespace std;
using namespace PgTools;
static void wr(const string &p, const void *d, size_t n) { ofstream f(p, ios::binary); f.write((const char *) d, n); }
static string rd(const string &p) { ifstream f(p, ios::binary); stringstream ss; ss << f.rdbuf(); return ss.str(); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const int L = atoi(argv[2]);
    const bool fast = atoi(argv[3]);
    const string cnt = rd(dir + "/cnt"), sym = rd(dir + "/sym"), off = rd(dir + "/off");
    PgHelpers::bytePerReadLengthMode = true;
    ReadsSetProperties props;
    props.readsCount = 0;
    props.allReadsLength = 0;
    props.constantReadLength = true;
    props.minReadLength = props.maxReadLength = L;
    props.symbolsCount = 4;
    strcpy(props.symbolsList, "ACGT");
    props.generateSymbolOrder();
    auto *rl = new ExtendedReadsListWithConstantAccessOption(L);
    SeparatedPseudoGenome sPg(string(cnt.size() + L, 'A'), rl, &props);
    ostringstream out;
    {
        SeparatedPseudoGenomeOutputBuilder builder(false, false);
        builder.copyPseudoGenomeProperties(&sPg);
        DefaultReadsListEntry e;
        size_t m = 0;
        for (size_t i = 0; i < cnt.size(); i++) {
            e.advanceEntryByOffset(1, (uint_reads_cnt_max) i, (i % 3) == 0);
            for (int k = 0; k < (uint8_t) cnt[i]; k++, m++) e.addMismatch((uint8_t) sym[m], (uint8_t) off[m]);
            builder.writeReadEntry(e);
        }
        builder.compressedBuild(out, fast ? CODER_LEVEL_FAST : CODER_LEVEL_NORMAL);
    }
    const string bytes = out.str();
    {   // the raw streams: order | props of the Pg, offsets, RC flags, zero flags, counts, codes, props, destinations
        istringstream in(bytes);
        char order[5];
        in.read(order, 5);
        wr(dir + "/order", order, 5);
        string s;
        readCompressed(in, s);
        const char *names[7] = {"rl_off", "rl_rc", "zero_flags", "nonzero_cnt", "codes", "props"};
        int limit = 0;
        for (int k = 0; k < 6; k++) {
            readCompressed(in, s);
            wr(dir + "/" + names[k], s.data(), s.size());
            if (k == 5) limit = (uint8_t) s[0];
        }
        for (int c = 1; c <= limit; c++) {
            readCompressed(in, s);
            wr(dir + "/dest" + to_string(c), s.data(), s.size());
        }
        if (in.peek() != EOF) { cerr << "bytes left in the archive" << endl; return 2; }
    }
    {   // the loader on the same bytes
        istringstream in(bytes);
        char order[5];
        in.read(order, 5);
        string ps;
        readCompressed(in, ps);
        istringstream pin(ps);
        PseudoGenomeHeader pgh(pin);
        ReadsSetProperties rsProp(pin);
        PgRCParams params;
        params.pgrcVersionMajor = PGRC_VERSION_MAJOR;
        params.pgrcVersionMinor = PGRC_VERSION_MINOR;
        auto *res = ExtendedReadsListWithConstantAccessOption::loadConstantAccessExtendedReadsList(in, &pgh, &rsProp, "", &params, false, false, false);
        wr(dir + "/loaded_cnt", res->misCnt.data(), res->misCnt.size());
        wr(dir + "/loaded_sym", res->misSymCode.data(), res->misSymCode.size());
        wr(dir + "/loaded_off", res->misOff.data(), res->misOff.size());
        delete res;
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


def forward_offsets(cnt, rev_off, L):
    """the ascending forward offsets whose rev-coding (writeReadEntry) is rev_off"""
    c = cnt.astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(c)])[:-1]
    eid = np.repeat(np.arange(c.size), c)
    k = np.arange(rev_off.size) - starts[eid]
    cs = np.cumsum(rev_off.astype(np.int64) + 1)
    fwd = L - (cs - np.concatenate([[0], cs])[starts[eid]])
    out = np.empty(rev_off.size, dtype=np.int64)
    out[starts[eid] + c[eid] - 1 - k] = fwd
    assert (out >= 0).all() and (out < L).all()
    return out.astype(np.uint8)


def reference_run(exe, tmp, cnt, sym, off, L, fast):
    for f in os.listdir(tmp):
        if f not in ("driver", "driver.cpp"):
            os.remove(os.path.join(tmp, f))
    for name, a in (("cnt", cnt), ("sym", sym), ("off", off)):
        a.tofile(os.path.join(tmp, name))
    subprocess.run([exe, tmp, str(L), str(int(fast))], check=True, stdout=subprocess.DEVNULL)
    return {f: np.fromfile(os.path.join(tmp, f), dtype=np.uint8) for f in os.listdir(tmp) if f not in ("driver", "driver.cpp", "cnt", "sym", "off")}


def main():
    manifest = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, seed, n, L, fast, knobs in CASES:
            cnt, sym, rev_off = la.make_list(seed, n, L, **knobs)
            if name == "ties":      # C and T exactly as often as each other, one A when the number is odd
                mv = np.tile(np.array([1, 3]), sym.size // 2 + 1)[:sym.size]
                mv[-1] = 0 if sym.size % 2 else mv[-1]
                sym = ((((mv + 1 + np.arange(sym.size) % 4) % 5) << 4) + mv).astype(np.uint8)
            off = forward_offsets(cnt, rev_off, L)
            assert np.array_equal(la.rev_offsets(cnt, off, L), rev_off)
            r = reference_run(exe, tmp, cnt, sym, off, L, fast)
            limit = int(r["props"][0])
            out = {"L": np.int64(L), "fast": np.int64(fast), "seed": np.int64(seed), "mis_cnt": cnt, "mis_sym": sym, "mis_off": off,
                   "knobs": np.frombuffer(json.dumps(knobs, sort_keys=True).encode(), dtype=np.uint8), "bases_order": r["order"]}
            for k in ("zero_flags", "nonzero_cnt", "codes", "props", "loaded_cnt", "loaded_sym", "loaded_off"):
                out[k] = r[k]
            for c in range(1, limit + 1):
                out[f"dest{c}"] = r[f"dest{c}"]
            # what the case stands for, from the reference's own streams
            lens = [0] + [int(r[f"dest{c}"].size) for c in range(1, limit + 1)]
            vals = np.bincount(sym & 15, minlength=5)[:5]
            info = dict(entries=n, L=L, fast=fast, mismatches=int(sym.size), zeros=int(r["zero_flags"].sum()), limit=limit, dest_len=lens,
                        order=r["order"].tobytes().decode(), value_counts=[int(v) for v in vals])
            assert r["zero_flags"].size == n and r["nonzero_cnt"].size == n - info["zeros"] and r["codes"].size == sym.size
            assert sum(lens) == sym.size and np.array_equal(r["loaded_cnt"], cnt) and np.array_equal(r["loaded_off"], off)
            if name == "mixed":
                assert 2 * info["zeros"] >= n and limit == 6 and lens[4] == 0 and all(lens[c] for c in (1, 2, 3, 5, 6)), info
                assert info["order"] != "ACGTN" and vals[4] > 0, info
            if name == "ties":
                assert vals[1] == vals[3] > vals[0] and info["order"].startswith("CT"), info
            if name == "no_mismatches":
                assert r["props"].tobytes() == b"\0" and sym.size == 0, info
            if name == "fast":
                assert r["props"].tobytes() == b"\1" and cnt.max() > 1 and lens[1] == sym.size, info
            if name == "max_one":
                assert r["props"].tobytes() == b"\1" and cnt.max() == 1, info
            if name == "wide":
                assert L == 255 and limit == 254 and lens[253] > 0 and lens[254] > 0, info
            if name == "one_entry":
                assert n == 1, info
            path = os.path.join(HERE, f"listarchive_{name}.npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes, the limit is {MAX_BYTES}"
            manifest[name] = dict(info, bytes=os.path.getsize(path))
            print(name, manifest[name])
    with open(os.path.join(HERE, "manifest_listarchive.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
