"""Writes tests/golden/huf_streams.npz: a handful of sources with the frames the compiled reference (oracle/_ref) makes of
them in Huffman mode -- FSECompress's frame (coders/FSECoder.cpp:34-78) around HUF_compress2's chunks, assembled here because
FSECompress gives the whole stream up where one chunk does not shrink; such a chunk is stored raw, which its reader takes.
The device tests decode these frames without the reference being present: its own FSE-coded weight headers, its other code
lengths, table log 12.

    python tests/golden/make_golden_huf.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import huf_util as hu  # noqa: E402

CASES = [("four", 5000, 12, 11), ("two", 3000, 10, 11), ("s129", 4099, 11, 11), ("s130", 4099, 11, 11), ("geo", 9000, 12, 11),
         ("fib", 8193, 12, 11), ("fib", 8193, 12, 12), ("geo", 4096, 12, 12), ("mixed", 9001, 10, 11)]


def ref_frame(x, order: int, table_log: int) -> bytes:
    chunks = []
    for c in hu.split(x, order):
        r = hu.ref_compress_chunk(c, table_log)
        chunks.append(c.tobytes() if r is None else r)
    return hu.frame(chunks, order, table_log)


def main() -> None:
    assert hu.ref_lib() is not None, "oracle/_ref/libpgrc_ref.so is not built"
    out = {}
    for i, (kind, n, order, tl) in enumerate(CASES):
        x = hu.mixed(n, order) if kind == "mixed" else hu.source(kind, n, seed=20 + i)
        f = ref_frame(x, order, tl)
        assert hu.decode(f, n) == x.tobytes()
        out[f"{i}/{kind}/{order}/{tl}/src"] = x
        out[f"{i}/{kind}/{order}/{tl}/frame"] = np.frombuffer(f, np.uint8)
    path = os.path.join(HERE, "huf_streams.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
