"""What the archive tests share: sources in the style of test_gpu_rsets.chain_records, FASTQ files of them, the compiled
reference's decoder (and encoder) in a child process, and an archive's parts as flat arrays for a fixture.

The reference's decoder calls exit() where it fails, so it never runs inside pytest:

    python tests/archive_util.py decode ARCHIVE                      -> ARCHIVE_out, or ARCHIVE_out_1 and ARCHIVE_out_2
    python tests/archive_util.py encode SRC PAIR|- ARCHIVE ORDER     -> ARCHIVE, by the reference's encoder at -t 1
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libpgrc_ref.so")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMPLEMENT = np.zeros(256, np.uint8)
COMPLEMENT[list(b"ACGTN")] = list(b"TGCAN")


def have_ref() -> bool:
    return os.path.exists(REF_LIB)


def make_reads(n=4000, L=100, coverage=20, seed=11, paired=False, noisy=True):
    """n reads of a random genome at the given coverage: about 1 % substitutions, every 100th read with one N, half of the
    fragments reverse-complemented; with `noisy`, as in chain_records, every 10th read has 12 symbols drawn anew, so that it
    neither overlaps nor maps, and every second read with an N has a second half that maps nowhere: the LQ and the N
    pseudogenome are not empty.  paired: the reads 2i and 2i + 1 are the two ends of one fragment of 2 L to 3 L symbols, the
    second end reverse-complemented (file 1 holds the even reads, file 2 the odd ones).  -> (n, L) uint8 rows"""
    rng = np.random.default_rng(seed)
    G = max(n * L // coverage, 4 * L)
    genome = ACGT[rng.integers(0, 4, size=G)]
    reads = np.empty((n, L), np.uint8)
    frags = n // 2 if paired else n
    flen = rng.integers(2 * L, 3 * L + 1, size=frags) if paired else np.full(frags, L)
    start = rng.integers(0, G - flen)
    flip = rng.random(frags) < 0.5
    for f in range(frags):
        frag = genome[start[f]: start[f] + flen[f]]
        if flip[f]:
            frag = COMPLEMENT[frag[::-1]]
        if paired:
            reads[2 * f], reads[2 * f + 1] = frag[:L], COMPLEMENT[frag[::-1][:L]]
        else:
            reads[f] = frag
    subst = rng.random((n, L)) < 0.01
    reads[subst] = ACGT[(np.searchsorted(ACGT, reads[subst]) + rng.integers(1, 4, size=int(subst.sum()))) % 4]
    idx = np.arange(n)
    with_n = idx % 100 == 7
    reads[with_n, rng.integers(0, L, size=int(with_n.sum()))] = ord("N")
    if noisy:
        for r in np.flatnonzero((idx % 10 == 3) & ~with_n):
            at = rng.choice(L, size=min(12, L), replace=False)
            reads[r, at] = ACGT[rng.integers(0, 4, size=at.size)]
        # every second read with an N: its second half complemented symbol by symbol, the N there too.  L / 2 mismatches are
        # more than any matcher allows, so the read stays in the N set; its first half is still the genome's, so that the N
        # pseudogenome has something to be mapped on the HQ one
        for r in np.flatnonzero(idx % 200 == 7):
            tail = reads[r, L // 2:]
            was_n = tail == ord("N")
            reads[r, L // 2:] = np.where(was_n, tail, COMPLEMENT[tail])
            if not was_n.any():
                reads[r, reads[r] == ord("N")] = ord("A")
                reads[r, L - 1 - (r % (L // 2))] = ord("N")
    return reads


def write_fastq(path, rows) -> None:
    L = rows.shape[1]
    qual = b"I" * L
    with open(path, "wb") as f:
        for i, r in enumerate(rows):
            f.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + qual + b"\n")


def write_text(path, rows, fmt: str) -> None:
    """the rows as FASTQ, as FASTA (a header line and the read) or one read per line"""
    if fmt == "fastq":
        return write_fastq(path, rows)
    with open(path, "wb") as f:
        for i, r in enumerate(rows):
            f.write((b">r%d\n" % i if fmt == "fasta" else b"") + r.tobytes() + b"\n")


def write_source(directory, reads, paired: bool, stem="in"):
    """-> (src, pair or None)"""
    if not paired:
        src = os.path.join(directory, stem + ".fastq")
        write_fastq(src, reads)
        return src, None
    src, pair = os.path.join(directory, stem + "_1.fastq"), os.path.join(directory, stem + "_2.fastq")
    write_fastq(src, reads[0::2])
    write_fastq(pair, reads[1::2])
    return src, pair


def read_rows(path, L: int) -> np.ndarray:
    """a decoder's output file (one read a line) -> (n, L) rows"""
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw.size % (L + 1) == 0, f"{path}: not lines of {L} symbols"
    rows = raw.reshape(-1, L + 1)
    assert (rows[:, L] == ord("\n")).all()
    return rows[:, :L]


def _child(*args) -> None:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"the reference's {args[0]} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"


def ref_decode(archive: str, paired: bool, L: int):
    """the compiled reference's decoder on `archive` -> the rows of its output file(s)"""
    names = [archive + "_out_1", archive + "_out_2"] if paired else [archive + "_out"]
    for n in names:
        if os.path.exists(n):
            os.remove(n)
    _child("decode", archive)
    return [read_rows(n, L) for n in names]


def ref_encode(src: str, pair, archive: str, preserve_order: bool) -> None:
    _child("encode", src, pair or "-", archive, int(preserve_order))


def ref_decoder():
    """the compiled reference's Uncompress (coders/CodersLib.cpp:251-292) as pgrc_amd.archive's decoder plug-in: what
    INTEGRATION.md §15 describes, taken from oracle/_ref instead of a caller's tree.  It exits on a damaged stream."""
    lib = C.CDLL(REF_LIB)
    un = lib._Z10UncompressPhmS_mhPSo                            # Uncompress(unsigned char*, size_t, unsigned char*, size_t, uint8_t, ostream*)
    un.argtypes, un.restype = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_uint8, C.c_void_p], None
    log = C.addressof(C.c_char.in_dll(lib, "null_stream"))

    def decoder(coder_type, payload, dest_len):
        out = C.create_string_buffer(dest_len)
        un(out, dest_len, payload, len(payload), coder_type, log)
        return out.raw[:dest_len]
    return decoder


def same_multiset(got_files, want_files) -> bool:
    """the rows of the files taken together as multisets; two files: the multisets of pairs, as the reference's -i src pair
    compares them (pgrc-decoder.cpp:670-686)"""
    got = np.concatenate(got_files, axis=1)
    want = np.concatenate(want_files, axis=1)
    if got.shape != want.shape:
        return False
    def order(a):
        return a[np.lexsort(a.T[::-1])]
    return bool(np.array_equal(order(got), order(want)))


def source_files(reads, paired: bool):
    return [reads[0::2], reads[1::2]] if paired else [reads]


# ---------------------------------------------------------------------------------------------------- parts <-> flat arrays
def flatten_parts(parts: dict, prefix: str) -> dict:
    """the parts pgrc_amd.archive.write_archive takes as named arrays for an .npz"""
    from pgrc_amd import archive as ar
    out = {}

    def put(key, v):
        out[f"{prefix}/{key}"] = np.frombuffer(ar._b(v), dtype=np.uint8).copy()
    out[f"{prefix}/header"] = np.array([parts["mode"], parts["read_length"], int(parts["rev_compl_pair_file"])], np.int64)
    for w in ar.LISTS:
        lst = parts[w]
        out[f"{prefix}/{w}/counts"] = np.array([lst["n_entries"], lst["pg_length"]], np.int64)
        if lst.get("off") is not None:
            put(f"{w}/off", lst["off"])
    hq = parts["hq"]
    put("hq/rev_comp", hq["rev_comp"])
    a = hq["archive"]
    for k in ("zero_flags", "nonzero_cnt", "mis_sym", "bases_order", "props"):
        put(f"hq/{k}", a[k])
    for c, d in enumerate(a["dests"]):
        if c:
            put(f"hq/dest{c:03d}", d)
    o = parts.get("order")
    if o:
        for k, v in o.items():
            if k not in ("n_total", "pos_width", "form"):
                put(f"order/{k}", v)
    g = parts["pgs"]
    out[f"{prefix}/pgs/mapped_lens"] = np.array(g["mapped_lens"], np.int64)
    put("pgs/book", g["mapped"].book)
    put("pgs/payload", g["mapped"].payload)
    for p, w in enumerate(ar.LISTS):
        put(f"pgs/{w}/map_off", g["map_off"][p])
        put(f"pgs/{w}/map_len", g["map_len"][p])
    return out


def unflatten_parts(z, prefix: str) -> dict:
    from pgrc_amd import archive as ar

    def get(key):
        return z[f"{prefix}/{key}"]
    mode, L, rc = (int(x) for x in get("header"))
    parts = {"mode": mode, "read_length": L, "rev_compl_pair_file": bool(rc), "separate_n": True, "name": "pgrc_amd"}
    for w in ar.LISTS:
        n, pg = (int(x) for x in get(f"{w}/counts"))
        parts[w] = {"n_entries": n, "pg_length": pg, "off": get(f"{w}/off") if f"{prefix}/{w}/off" in z else None}
    dests = [np.zeros(0, np.uint8)] + [z[k] for k in sorted(z.files) if k.startswith(f"{prefix}/hq/dest")]
    parts["hq"]["rev_comp"] = get("hq/rev_comp")
    parts["hq"]["archive"] = dict({k: get(f"hq/{k}") for k in ("zero_flags", "nonzero_cnt", "mis_sym", "props")},
                                  bases_order=get("hq/bases_order").tobytes(), dests=dests)
    parts["order"] = {k.split("/")[-1]: z[k] for k in z.files if k.startswith(f"{prefix}/order/")} or None
    lens = tuple(int(x) for x in get("pgs/mapped_lens"))
    parts["pgs"] = {"mapped_lens": lens, "mapped": ar.VarLenCoded(get("pgs/book").tobytes(), get("pgs/payload"), sum(lens)),
                    "map_off": [get(f"pgs/{w}/map_off") for w in ar.LISTS], "map_len": [get(f"pgs/{w}/map_len") for w in ar.LISTS]}
    return parts


def main(argv) -> int:
    lib = C.CDLL(REF_LIB)
    if argv[0] == "decode":
        lib.pgrc_ref_decode.argtypes = [C.c_char_p, C.c_int]
        return lib.pgrc_ref_decode(argv[1].encode(), 1)
    if argv[0] == "encode":
        lib.pgrc_ref_encode.argtypes = [C.c_char_p] * 3 + [C.c_int] * 3 + [C.c_char, C.c_int, C.c_int, C.c_char, C.c_int]
        pair = b"" if argv[2] == "-" else argv[2].encode()
        r = lib.pgrc_ref_encode(argv[1].encode(), pair, argv[3].encode(), 1, 0, int(argv[4]), b"\0", 0, 0, b"\0", 0)
        return 0 if r >= 0 else 1
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
