"""Records the raw streams of two small archives for tests/test_archive_container.py: needs an MI355X.

    python tests/golden/make_golden_archive.py [OUT.npz]            (default: tests/golden/archive_streams.npz)

600 reads of 40 bp from an 8 kbp genome (archive_util.make_reads at coverage 3, a few with N), once single-end without the
order and once paired with it, go through pgrc_amd.pipeline.compress_parts; what would go into the file is stored as flat
arrays (archive_util.flatten_parts) beside the source reads.  Before anything is stored each archive is written, read back
and verified against its source on the device."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import archive_util as au  # noqa: E402
from pgrc_amd import archive as ar, pipeline  # noqa: E402

CASES = (("golden_se", 5, False, False), ("golden_ord_pe", 6, True, True))


def main(out_path: str) -> None:
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, seed, paired, order in CASES:
            reads = au.make_reads(600, 40, coverage=3, seed=seed, paired=paired)
            src, pair = au.write_source(d, reads, paired, stem=name)
            parts, report = pipeline.compress_parts(src, pair, order)
            arc = os.path.join(d, name + ".pgrc")
            ar.write_archive(arc, parts)
            dec, _ = pipeline.load(arc)
            with dec.verifier() as v:
                for f, rows in enumerate(au.source_files(reads, paired)):
                    v.add_rows(f, np.ascontiguousarray(rows))
                assert v.finish()["ok"], name
            dec.close()
            assert all(report["counts"]) and (reads == ord("N")).any(), (name, report)
            out.update(au.flatten_parts(parts, name))
            out[name + "/reads"] = reads
            print(name, report)
    np.savez_compressed(out_path, **out)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "archive_streams.npz"))
