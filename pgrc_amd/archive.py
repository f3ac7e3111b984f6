"""The PgRC archive as a container: the file header, the framing of its streams and the order of its parts, restated from
the reference's writer and readers.  Plain host Python; no device code, and no coder of the reference: coders are a plug-in.

    writer    coder(stream_name, data) -> (coder_type, payload)           None, or a payload not shorter than data: stored raw
    reader    decoder(coder_type, payload, dest_len) -> bytes             asked for every stream that is not stored raw

The file (pgrc/pgrc-encoder.cpp:27-54, :92-93; pgrc/pgrc-decoder.cpp:14-60):

    "PgRC" '#' major minor revision level mode separateNReads [revComplPairFile: PE and ORD_PE only] name '\\n'

and behind it (pgrc-decoder.cpp:727-827, loadAllPgs) five raw bytes, the HQ list's basesOrdered
(SeparatedPseudoGenomePersistence.cpp:941-942), and then nothing but framed streams, one after the other: the decoder
prefetches them all as such (CodersLib.cpp:542-547).  Their order is PARTS below.

One stream (writeCompressed / writeHeader, CodersLib.cpp:294-334; readCompressed, :345-381; the collective forms :503-540 and
:549-641 write and read the same bytes, one job after the other):

    u64 0                                                        an empty stream: a lone zero length
    u64 dest_len, u64 src_len, u8 coder_type, src_len bytes      NO_CODER (0): src_len == dest_len, the bytes as they are
    u64 dest_len, u64 inner_len, u8 77, u64 comp_len, u8 primary_type, inner_len bytes
                                                                 the compound form: the inner bytes are one framed stream of
                                                                 comp_len bytes (the secondary coder's), which the primary
                                                                 coder takes back to dest_len bytes; inner_len is the inner
                                                                 payload plus its 17 header bytes (CoderProps::getHeaderLen)

A var-len DNA coded stream (type 11; VarLenDNACoder::Compress, coders/VarLenDNACoder.cpp:122-154; ::Uncompress, :160-181) is
two bytes (the mode, the static book's id), the book as writeBook wrote it (every code and '\\n', the last one NUL) and the
codes.  The container neither codes nor decodes it: VarLenCoded carries its parts to and from pgrc_amd.VarLenDNACoder.
"""
from __future__ import annotations

import io
import struct
from typing import Callable, Optional

import numpy as np

NO_CODER, LZMA_CODER, LZMA2_CODER, PPMD7_CODER, RANGE_CODER, FSE_HUF_CODER = 0, 1, 2, 3, 4, 5       # coders/CodersLib.h:16-25
VARLEN_DNA_CODER, COMPOUND_CODER_TYPE, PARALLEL_BLOCKS_CODER_TYPE, SELECTOR_CODER_TYPE = 11, 77, 88, 99
CODER_NAMES = {NO_CODER: "NO_CODER", LZMA_CODER: "LZMA", LZMA2_CODER: "LZMA2", PPMD7_CODER: "PPMd7", RANGE_CODER: "range coder",
               FSE_HUF_CODER: "FSE/Huffman", VARLEN_DNA_CODER: "var-len DNA", COMPOUND_CODER_TYPE: "compound",
               PARALLEL_BLOCKS_CODER_TYPE: "parallel blocks", SELECTOR_CODER_TYPE: "selector"}

PGRC_HEADER = b"PgRC"                                            # pgrc/pgrc-params.h:11-27
PGRC_VERSION_MODE = ord("#")
PGRC_VERSION = (2, 0, 2)
PGRC_SE_MODE, PGRC_PE_MODE, PGRC_ORD_SE_MODE, PGRC_ORD_PE_MODE, PGRC_MIN_PE_MODE = 0, 1, 2, 3, 4
MODE_NAMES = {PGRC_SE_MODE: "SE", PGRC_PE_MODE: "PE", PGRC_ORD_SE_MODE: "ORD_SE", PGRC_ORD_PE_MODE: "ORD_PE", PGRC_MIN_PE_MODE: "MIN_PE"}
CODER_LEVEL_FAST, CODER_LEVEL_NORMAL, CODER_LEVEL_MAX = 1, 2, 3  # coders/CodersLib.h:33-35
STREAM_HEADER_LEN = 17                                           # CoderProps::getHeaderLen, coders/CodersLib.h:58
VAR_LEN_PROPS_SIZE = 2                                           # coders/VarLenDNACoder.h
PSEUDOGENOME_HEADER = "PGEN"                                     # pgrc/pg-config.cpp:7
PG_TYPE = "SEPARATED_PGEN"                                       # PGTYPE_SEPARATED, pseudogenome/SeparatedPseudoGenome.h:10
EMPTY_BASES_ORDER = b"ACGNT"                                     # reorderingSymbolsExclusiveMismatchEncoding of no symbol (:1115-1138)

PAIRED_MODES = (PGRC_PE_MODE, PGRC_ORD_PE_MODE)
ORD_MODES = (PGRC_ORD_SE_MODE, PGRC_ORD_PE_MODE)


class ArchiveError(ValueError):
    """a file that is no PgRC archive, is cut short, or holds a stream this reader has no decoder for"""


class VarLenCoded:
    """what VarLenDNACoder::Compress wrote, in parts: the two header bytes, the book (writeBook's bytes without the NUL) and
    the codes; dest_len is the length of the text the codes stand for"""

    def __init__(self, book: bytes, payload, dest_len: int, mode: int = 0, book_id: int = 0):
        self.book = bytes(book).rstrip(b"\0")
        self.payload = _b(payload)
        self.dest_len, self.mode, self.book_id = int(dest_len), int(mode), int(book_id)

    def to_bytes(self) -> bytes:
        return bytes([self.mode, self.book_id]) + self.book + b"\0" + self.payload

    @classmethod
    def from_bytes(cls, raw: bytes, dest_len: int, name: str = "stream") -> "VarLenCoded":
        end = raw.find(b"\0", VAR_LEN_PROPS_SIZE)                # readBook: a C string (:156-158)
        if len(raw) < VAR_LEN_PROPS_SIZE + 1 or end < 0:
            raise ArchiveError(f"{name}: a var-len DNA stream without its book")
        return cls(raw[VAR_LEN_PROPS_SIZE:end], raw[end + 1:], dest_len, raw[0], raw[1])

    def __eq__(self, other):
        return isinstance(other, VarLenCoded) and (self.book, self.payload, self.dest_len, self.mode, self.book_id) == \
            (other.book, other.payload, other.dest_len, other.mode, other.book_id)

    def __len__(self):
        return self.dest_len


def _b(a) -> bytes:
    if a is None:
        return b""
    if isinstance(a, (bytes, bytearray, memoryview)):
        return bytes(a)
    if isinstance(a, str):
        return a.encode("latin-1")
    return np.ascontiguousarray(a).tobytes()


# ---------------------------------------------------------------------------------------------------- the framing
def write_stream(out, name: str, data, coder: Optional[Callable] = None) -> None:
    """writeCompressed (CodersLib.cpp:294-309) of one stream; a VarLenCoded goes out in the compound form with a secondary
    stage that `coder` may code (the reference's is LZMA or PPMd) and that is stored raw otherwise"""
    if isinstance(data, VarLenCoded):
        _write_compound(out, name, data, coder)
        return
    data = _b(data)
    if not data:
        out.write(struct.pack("<Q", 0))
        return
    ctype, payload = NO_CODER, data
    if coder is not None:
        res = coder(name, data)
        if res is not None:
            ctype, payload = int(res[0]), _b(res[1])
            if ctype == NO_CODER or len(payload) >= len(data):   # writeHeader: what does not shrink is stored (:326-328)
                ctype, payload = NO_CODER, data
    out.write(struct.pack("<QQB", len(data), len(payload), ctype))
    out.write(payload)


def _write_compound(out, name: str, v: VarLenCoded, coder) -> None:
    """writeHeader's compound branch (:317-325): the primary stage is done (v), the secondary one is this function's"""
    if v.dest_len == 0:
        out.write(struct.pack("<Q", 0))
        return
    comp = v.to_bytes()
    inner = io.BytesIO()
    write_stream(inner, name, comp, coder)
    inner = inner.getvalue()
    # (the reference stores the text itself where the primary stage does not shrink it and says NO_CODER (:160-163, :323-324);
    #  a stream that carries its book is written as what it is)
    out.write(struct.pack("<QQBQB", v.dest_len, len(inner), COMPOUND_CODER_TYPE, len(comp), VARLEN_DNA_CODER))
    out.write(inner)


def write_collective(out, jobs, coder: Optional[Callable] = None) -> None:
    """CompressionJob::writeCompressedCollectiveParallel (CodersLib.cpp:503-540): the jobs' streams one after the other;
    jobs: (name, data) pairs"""
    for name, data in jobs:
        write_stream(out, name, data, coder)


class StreamReader:
    """readCompressed and readCompressedCollectiveParallel over a file object: the streams come in file order and carry the
    names the caller gives them"""

    def __init__(self, src, decoder: Optional[Callable] = None):
        self.src, self.decoder = src, decoder

    def _take(self, n: int, name: str) -> bytes:
        b = self.src.read(n)
        if len(b) != n:
            raise ArchiveError(f"{name}: the archive ends inside the stream ({len(b)} of {n} bytes)")
        return b

    def _decode(self, name: str, ctype: int, payload: bytes, dest_len: int) -> bytes:
        if ctype == NO_CODER:                                    # NoCoderUncompress (:233-238)
            if len(payload) != dest_len:
                raise ArchiveError(f"{name}: a raw stream of {len(payload)} bytes for {dest_len}")
            return payload
        if self.decoder is None:
            raise ArchiveError(f"stream '{name}' is coded with coder type {ctype} ({CODER_NAMES.get(ctype, 'unknown')}) "
                               "and no decoder was given")
        got = self.decoder(ctype, payload, dest_len)
        if got is None:
            raise ArchiveError(f"stream '{name}': the decoder has no coder of type {ctype} ({CODER_NAMES.get(ctype, 'unknown')})")
        got = _b(got)
        if len(got) != dest_len:
            raise ArchiveError(f"stream '{name}': the decoder of type {ctype} gave {len(got)} bytes for {dest_len}")
        return got

    def read(self, name: str):
        """one stream -> its bytes, or a VarLenCoded for a compound stream whose primary coder is the var-len DNA coder"""
        (dest_len,) = struct.unpack("<Q", self._take(8, name))
        if dest_len == 0:
            return b""
        src_len, ctype = struct.unpack("<QB", self._take(9, name))
        if ctype != COMPOUND_CODER_TYPE:
            return self._decode(name, ctype, self._take(src_len, name), dest_len)
        comp_len, primary = struct.unpack("<QB", self._take(9, name))
        inner = StreamReader(io.BytesIO(self._take(src_len, name)), self.decoder)
        comp = inner.read(name)
        if isinstance(comp, VarLenCoded) or len(comp) != comp_len:
            raise ArchiveError(f"{name}: the compound stream's component has {len(comp)} bytes, not {comp_len}")
        if primary == VARLEN_DNA_CODER:
            return VarLenCoded.from_bytes(comp, dest_len, name)
        return self._decode(name, primary, comp, dest_len)

    def read_collective(self, names):
        return [self.read(n) for n in names]

    def at_end(self) -> bool:
        b = self.src.read(1)
        if b:
            self.src.seek(-1, io.SEEK_CUR)
        return not b


# ---------------------------------------------------------------------------------------------------- the properties
def pg_props(read_length: int, reads_count: int, pg_length: int, symbols: bytes) -> bytes:
    """buildProps and writeReadMode(.., false) (SeparatedPseudoGenomePersistence.cpp:759-770, :908): PseudoGenomeHeader::write
    (pseudogenome/PseudoGenomeBase.h:89-97), ReadsSetProperties::write (readsset/ReadsSetBase.h:66-74), "BIN" """
    L, n = int(read_length), int(reads_count)
    sym = _b(symbols).decode()
    return (f"{PSEUDOGENOME_HEADER}\n{PG_TYPE}\n1\n{L}\n{n}\n{int(pg_length)}\n"
            f"{n}\n{n * L}\n1\n{L}\n{L}\n{len(sym)}\n{sym}\nBIN\n").encode()


def parse_pg_props(raw: bytes, name: str = "props") -> dict:
    t = raw.decode("latin-1").split()
    try:
        if t[0] != PSEUDOGENOME_HEADER or t[-1] not in ("BIN", "TXT"):
            raise IndexError
        # a set without a read has no symbol: its list line is empty and the split drops it
        return {"type": t[1], "read_length": int(t[3]), "reads_count": int(t[4]), "pg_length": int(t[5]),
                "symbols": t[12].encode() if len(t) > 13 else b"", "text_mode": t[-1] == "TXT"}
    except (IndexError, ValueError):
        raise ArchiveError(f"{name}: not a pseudogenome's properties") from None


# ---------------------------------------------------------------------------------------------------- the parts
PAIRORDER_NAMES = ("off8_flag", "off_value", "delta8_flag", "delta_value", "full_offset")     # compressReadsOrder's jobs (:297-335)
PAIRORDER_FLAG_NAMES = ("off_base_file_flag", "nonoff_base_file_flag")
PAIRORDER_DTYPES = {"off8_flag": np.uint8, "off_value": np.uint8, "delta8_flag": np.uint8, "delta_value": np.int8,
                    "full_offset": np.uint32, "pair_base_org_idx": np.uint32, "off_base_file_flag": np.uint8,
                    "nonoff_base_file_flag": np.uint8}
PAIRPOS_NAMES = ("base_pos", "off16_flag", "off_base_first", "off_value", "delta16_flag", "delta_base_first", "delta_value",
                 "not_base_pos")                                                              # compressReadsPgPositions' (:532-570)
PAIRPOS_DTYPES = {"off16_flag": np.uint8, "off_base_first": np.uint8, "off_value": np.uint16, "delta16_flag": np.uint8,
                  "delta_base_first": np.uint8, "delta_value": np.int16}
LISTS = ("hq", "lq", "n")
LIST_SYMBOLS = {"hq": b"ACGT", "lq": b"ACGT", "n": b"ACGNT"}

PARTS = """the streams behind the five raw bytes, in file order (the names are the ones errors and coders see):
  hq.props [hq.off] hq.rev_comp hq.zero_flags hq.nonzero_cnt hq.mis_sym      compressedBuild (:905-947); no off in the ORD modes
  hq.mis_props hq.mis_off.1 .. hq.mis_off.n                                  compressRlMisRevOffDest (:823-903)
  lq.props [lq.off]   and, with separateNReads,   n.props [n.off]            compressedBuild of a list without the other streams
  order.*                                                                    PE: compressReadsOrder's five streams and two file-flag
                                                                             streams; ORD_SE: order.positions; ORD_PE: the eight of
                                                                             compressReadsPgPositions; SE: none
  pgs.lengths pgs.mapped pgs.hq.map_off pgs.hq.map_len pgs.lq.map_off pgs.lq.map_len [pgs.n.map_off pgs.n.map_len]
                                                                             matchPgsInPg (SimplePgMatcher.cpp:208-256)"""


def _list_jobs(which: str, lst: dict, ord_mode: bool, read_length: int):
    jobs = [(f"{which}.props", pg_props(read_length, lst["n_entries"], lst["pg_length"], LIST_SYMBOLS[which]))]
    if not ord_mode:
        jobs.append((f"{which}.off", lst["off"]))
    if which != "hq":
        return jobs, []
    a = lst["archive"]
    jobs += [("hq.rev_comp", lst["rev_comp"]), ("hq.zero_flags", a["zero_flags"]), ("hq.nonzero_cnt", a["nonzero_cnt"]),
             ("hq.mis_sym", a["mis_sym"])]
    dests = a["dests"]
    n_dests = len(dests) - 1
    if len(_b(a["props"])) < 1 or _b(a["props"])[0] != n_dests:
        raise ArchiveError("hq: the mismatch properties do not name the number of offset streams")
    return jobs, [("hq.mis_props", a["props"])] + [(f"hq.mis_off.{c}", dests[c]) for c in range(1, n_dests + 1)]


def write_archive(path, parts: dict, coder: Optional[Callable] = None) -> int:
    """the archive of `parts` (as read_archive returns them) -> its size.  Written under a temporary name and renamed, as
    finalizeCompression does (pgrc-encoder.cpp:497-509)."""
    import os
    mode = int(parts["mode"])
    if mode not in MODE_NAMES or mode == PGRC_MIN_PE_MODE:
        raise ArchiveError(f"archive mode {mode} is not written (SE, PE, ORD_SE and ORD_PE are)")
    sep_n = bool(parts.get("separate_n", True))
    ord_mode, paired = mode in ORD_MODES, mode in PAIRED_MODES
    L = int(parts["read_length"])
    tmp = str(path) + ".temp"
    with open(tmp, "wb") as out:
        out.write(PGRC_HEADER + bytes([PGRC_VERSION_MODE, *PGRC_VERSION, int(parts.get("compression_level", CODER_LEVEL_NORMAL)),
                                       mode, int(sep_n)]))
        if mode in (PGRC_PE_MODE, PGRC_ORD_PE_MODE):
            out.write(bytes([int(bool(parts.get("rev_compl_pair_file", True)))]))
        name = parts.get("name", "pgrc_amd")
        if not name or any(c.isspace() for c in name):
            raise ArchiveError("the archive's name line is one word")      # (the decoder reads it with >> : pgrc-decoder.cpp:46)
        out.write(name.encode() + b"\n")
        bases_order = bytes(parts["hq"]["archive"]["bases_order"])
        if len(bases_order) != 5:
            raise ArchiveError("basesOrdered is five bytes")
        out.write(bases_order)
        first, second = _list_jobs("hq", parts["hq"], ord_mode, L)
        write_collective(out, first, coder)
        write_collective(out, second, coder)
        for which in ("lq", "n") if sep_n else ("lq",):
            write_collective(out, _list_jobs(which, parts[which], ord_mode, L)[0], coder)
        o = parts.get("order")
        if mode == PGRC_ORD_SE_MODE:
            write_stream(out, "order.positions", o["positions"], coder)
        elif mode == PGRC_ORD_PE_MODE:
            write_collective(out, [(f"order.{k}", o[k]) for k in PAIRPOS_NAMES], coder)
        elif mode == PGRC_PE_MODE:
            write_collective(out, [(f"order.{k}", o[k]) for k in PAIRORDER_NAMES + PAIRORDER_FLAG_NAMES], coder)
        g = parts["pgs"]
        jobs = [("pgs.lengths", struct.pack("<3Q", *[int(x) for x in g["mapped_lens"]])), ("pgs.mapped", g["mapped"])]
        for p, which in enumerate(LISTS if sep_n else LISTS[:2]):
            jobs += [(f"pgs.{which}.map_off", g["map_off"][p]), (f"pgs.{which}.map_len", g["map_len"][p])]
        write_collective(out, jobs, coder)
        size = out.tell()
    os.replace(tmp, str(path))
    return size


def read_header(src) -> dict:
    """pgrc-decoder.cpp:14-49; archives from before the version bytes (no '#') are refused"""
    head = src.read(len(PGRC_HEADER) + 1)
    if head[:4] != PGRC_HEADER or len(head) != 5:
        raise ArchiveError("not a PgRC archive: the header is missing")
    if head[4] != PGRC_VERSION_MODE:
        raise ArchiveError("a PgRC archive from before version 1.2 (no version bytes): not supported")
    b = src.read(6)
    if len(b) != 6:
        raise ArchiveError("the archive ends inside its header")
    major, minor, rev, level, mode, sep_n = b
    if (major, minor) > PGRC_VERSION[:2]:
        raise ArchiveError(f"the archive is packed with a newer PgRC version {major}.{minor}")
    if (major, minor) < (1, 3):
        raise ArchiveError(f"a PgRC {major}.{minor} archive: the stream layout of 1.3 and later is the one supported")
    if mode not in MODE_NAMES:
        raise ArchiveError(f"unsupported decompression mode: {mode}")
    if mode == PGRC_MIN_PE_MODE:
        raise ArchiveError("a PGRC_MIN_PE_MODE archive (written with the pair order ignored): not supported")
    h = {"version": (major, minor, rev), "compression_level": level, "mode": mode, "separate_n": bool(sep_n),
         "rev_compl_pair_file": False}
    if mode in (PGRC_PE_MODE, PGRC_ORD_PE_MODE):
        flag = src.read(1)
        if not flag:
            raise ArchiveError("the archive ends inside its header")
        h["rev_compl_pair_file"] = bool(flag[0])
    name = bytearray()
    while True:
        c = src.read(1)
        if not c:
            raise ArchiveError("the archive ends inside its header")
        if c == b"\n":
            break
        name += c
    h["name"] = name.decode("latin-1")
    return h


def read_archive(path, decoder: Optional[Callable] = None) -> dict:
    """loadAllPgs (pgrc-decoder.cpp:727-827) and restoreMatchedPgs' reading part (SimplePgMatcher.cpp:259-286) -> the parts:
    the header's fields, read_length, hq / lq / n (n_entries, pg_length, off, and for hq rev_comp and archive, the dict
    PgRCDecoder.add_list_archive takes), order (the dict the decoder's set_order_* calls take, None for SE) and pgs
    (mapped_lens, mapped: bytes or a VarLenCoded, map_off and map_len: three each)"""
    with open(path, "rb") as src:
        parts = read_header(src)
        mode, sep_n = parts["mode"], parts["separate_n"]
        ord_mode = mode in ORD_MODES
        bases_order = src.read(5)
        if len(bases_order) != 5:
            raise ArchiveError("the archive ends before its first stream")
        r = StreamReader(src, decoder)
        for which in LISTS if sep_n else LISTS[:2]:
            p = parse_pg_props(r.read(f"{which}.props"), f"{which}.props")
            if p["text_mode"]:
                raise ArchiveError("reads list text mode unsupported during decompression")
            lst = {"n_entries": p["reads_count"], "pg_length": p["pg_length"], "read_length": p["read_length"], "off": None}
            wide = p["read_length"] > 255
            if not ord_mode:
                lst["off"] = np.frombuffer(r.read(f"{which}.off"), dtype=np.uint16 if wide else np.uint8)
            if which == "hq":
                lst["rev_comp"] = np.frombuffer(r.read("hq.rev_comp"), dtype=np.uint8)
                a = {"zero_flags": r.read("hq.zero_flags"), "nonzero_cnt": r.read("hq.nonzero_cnt"), "mis_sym": r.read("hq.mis_sym"),
                     "bases_order": bases_order, "props": r.read("hq.mis_props")}
                if not a["props"]:
                    raise ArchiveError("hq.mis_props: empty")
                a["dests"] = [b""] + [r.read(f"hq.mis_off.{c}") for c in range(1, a["props"][0] + 1)]
                lst["archive"] = {k: (np.frombuffer(v, dtype=np.uint8) if isinstance(v, bytes) and k != "bases_order" else v)
                                  for k, v in a.items()}
                lst["archive"]["dests"] = [np.frombuffer(d, dtype=np.uint8) for d in a["dests"]]
            parts[which] = lst
        if not sep_n:
            parts["n"] = {"n_entries": 0, "pg_length": 0, "read_length": parts["hq"]["read_length"], "off": None if ord_mode else np.zeros(0, np.uint8)}
        parts["read_length"] = parts["hq"]["read_length"]
        total = sum(parts[w]["n_entries"] for w in LISTS)
        joined = sum(parts[w]["pg_length"] for w in LISTS)
        width = 4 if joined <= 0xFFFFFFFF else 8                 # isJoinedPgLengthStd (:805)
        pos_t = np.uint32 if width == 4 else np.uint64
        parts["n_total"] = total
        if mode == PGRC_SE_MODE:
            parts["order"] = None
        elif mode == PGRC_ORD_SE_MODE:
            parts["order"] = {"positions": np.frombuffer(r.read("order.positions"), dtype=pos_t)}
        elif mode == PGRC_ORD_PE_MODE:
            o = {"n_total": total, "pos_width": width}
            for k in PAIRPOS_NAMES:
                o[k] = np.frombuffer(r.read(f"order.{k}"), dtype=PAIRPOS_DTYPES.get(k, pos_t))
            parts["order"] = o
        else:
            o = {"n_total": total, "form": 1}                    # PGRC_PAIRORDER_FILE_FLAGS (include/pgrc_decode.h)
            for k in PAIRORDER_NAMES + PAIRORDER_FLAG_NAMES:
                o[k] = np.frombuffer(r.read(f"order.{k}"), dtype=PAIRORDER_DTYPES[k])
            parts["order"] = o
        lens = r.read("pgs.lengths")
        if len(lens) != 24:
            raise ArchiveError("pgs.lengths: three 64-bit lengths expected")
        g = {"mapped_lens": struct.unpack("<3Q", lens), "mapped": r.read("pgs.mapped"), "map_off": [b"", b"", b""], "map_len": [b"", b"", b""]}
        if len(g["mapped"]) != sum(g["mapped_lens"]):
            raise ArchiveError("pgs.mapped: its length is not the sum of the three mapped lengths")
        for p, which in enumerate(LISTS):
            if p == 2 and r.at_end():                            # (written with separateNReads, :248-255; read only for a text, :282-285)
                break
            g["map_off"][p], g["map_len"][p] = r.read(f"pgs.{which}.map_off"), r.read(f"pgs.{which}.map_len")
        parts["pgs"] = g
        parts["bytes_left"] = len(src.read())                    # 0: the file ends with its last stream
    return parts
