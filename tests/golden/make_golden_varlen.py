#!/usr/bin/env python3
"""Golden fixtures of the variable-length DNA coder (pgrc_varlen_encode / _decode), made by the REAL reference compiled in
the build container (oracle/_ref/libpgrc_ref.so).

A throwaway C++ driver, compiled in a temporary directory against that library and the reference's headers, pushes a text
through VarLenDNACoder::Compress with each of the three static book ids and takes it back through ::Uncompress.  Fixtures
are data only: where the text comes from (a generator of tests/varlen_util.py with its seed and length, or a pgmap_*
fixture whose mapped parts are joined), its digest, and the reference's whole output per book id: the two header bytes,
the book as writeBook wrote it, the payload.  The pgmap-derived texts are recorded with the encoder's book (id 0) only, which
keeps the set to a few hundred KB.

A text shorter than 4 symbols is not recorded: the reference's `srcLen - 4` wraps there and its loop runs off the text, so
it has no output to record (the driver is started for n = 3 and its failure is noted in the manifest).  That case is defined
by include/pgrc_varlen.h and checked against tests/varlen_util.encode_serial.

    python tests/golden/make_golden_varlen.py        # needs the reference tree (run `make -C oracle ref` first)
"""
import glob
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

import varlen_util as vu  # noqa: E402

REF = os.environ.get("PGRC_REFERENCE", "/root/reference")

DRIVER = r"""
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "coders/VarLenDNACoder.h"
using namespace std;
static string rd(const string &p) { ifstream f(p, ios::binary); stringstream s; s << f.rdbuf(); return s.str(); }
static void wr(const string &p, const string &s) { ofstream f(p, ios::binary); f.write(s.data(), s.size()); }
int main(int argc, char **argv) {
    const string dir = argv[1];
    const string text = rd(dir + "/text");
    for (int a = 2; a < argc; a++) {
        const int id = atoi(argv[a]);
        PgHelpers::VarLenDNACoderProps props((uint8_t) id);
        unsigned char *dest = nullptr;
        size_t destLen = 0;
        PgHelpers::VarLenDNACoder::Compress(dest, destLen, (const unsigned char *) text.data(), text.size(), &props);
        wr(dir + "/coded" + to_string(id), string((const char *) dest, destLen));
        string back(text.size(), '\0');
        size_t backLen = back.size();
        PgHelpers::VarLenDNACoder::Uncompress((unsigned char *) &back[0], &backLen, dest, destLen);
        if (back != text) { cerr << "Uncompress differs from the text" << endl; return 2; }
        delete[] dest;
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
    subprocess.run(["g++", "-std=c++17", "-O2", "-w", "-I" + REF, src, "-o", exe, "-L" + refdir, "-lpgrc_ref",
                    "-Wl,-rpath," + refdir], check=True)
    return exe


def main():
    manifest = {}
    cases = [(name, f"{kind}:{seed}:{n}", vu.make_text(kind, seed, n), vu.BOOK_IDS) for name, kind, seed, n in vu.TEXT_CASES]
    for path in sorted(glob.glob(os.path.join(HERE, "pgmap_*.npz"))):
        stem = os.path.basename(path)[:-4]
        cases.append((stem, stem, vu.joined_mapped(np.load(path)), (0,)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, source, text, ids in cases:
            text.tofile(os.path.join(tmp, "text"))
            if text.size < 4:
                try:
                    r = subprocess.run([exe, tmp, "0"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=20)
                    how = f"exit status {r.returncode}"
                except subprocess.TimeoutExpired:
                    how = "no return within 20 s"
                manifest[name] = {"symbols": int(text.size), "recorded": False, "reference": how}
                print(name, manifest[name])
                continue
            subprocess.run([exe, tmp] + [str(i) for i in ids], check=True, stdout=subprocess.DEVNULL)
            out = {"source": np.frombuffer(source.encode(), np.uint8), "digest": np.frombuffer(vu.digest(text).encode(), np.uint8)}
            entry = {"symbols": int(text.size), "recorded": True, "payload_bytes": {}, "ratio": {}}
            for i in ids:
                coded = np.fromfile(os.path.join(tmp, f"coded{i}"), dtype=np.uint8)
                mode, bid, book, payload = vu.parse_stream(coded)
                assert (mode, bid) == (0, i) and vu.decode(book, payload) == text.tobytes()
                out[f"coded{i}"] = coded
                entry["payload_bytes"][str(i)] = len(payload)
                entry["ratio"][str(i)] = round(len(payload) / text.size, 4)
            np.savez_compressed(os.path.join(HERE, f"varlen_{name}.npz"), **out)
            manifest[name] = entry
            print(name, entry)
    with open(os.path.join(HERE, "manifest_varlen.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
