"""The two drivers: reads in, archive out (`compress`); archive in, reads out (`decompress`).  Each runs the reference's
stage order (PgRCEncoder::executePgRCChain, pgrc/pgrc-encoder.cpp:108-252; PgRCDecoder::decompressPgRC,
pgrc/pgrc-decoder.cpp:7-98) on the package's device objects and leaves the file itself to pgrc_amd.archive.  No compute here:
what comes down from the device is what goes into the file, and the counts that steer the stages.

The parameters are the reference's defaults (PgRCParams::initCompressionParameters, pgrc/pgrc-params.h:115-151): quality
division at 120 promils with the simplified suffix rule, generator division at 65 %, matching mode 'c' with seed 38 and 3
characters per mismatch, Pg-vs-Pg matches of 45 and more; N reads in a set of their own, the pair file reverse-complemented.
PGRC_MIN_PE_MODE and the expert options are not offered.

The var-len DNA book.  The joined mapped text goes through pgrc_amd.VarLenDNACoder, and the stream carries its book, so any
valid book decodes everywhere.  `default_book()` makes one of this package's own (the reference's books are text of its
source and are not repeated here); a caller with another book passes `book=`.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
from typing import Callable, Optional

import numpy as np

from . import _lib, archive as ar
from ._lib import MatchParams, PgrcMatchError, lib
from .assemble import PgAssembler
from .decode import PGRC_DECODE_SE, PGRC_PAIRORDER_FILE_FLAGS, PgRCDecoder
from .matchers import MatchContext
from .overlap import OverlapFinder
from .readsets import DividedPCLReadsSets, DividedReadsSets, reads_text_format
from .rlist import ReadsList
from .textmatch import CopMEMMatcher
from .varlen import VarLenDNACoder

# PgRCParams::initCompressionParameters, CODER_LEVEL_NORMAL (pgrc-params.h:138-146)
ERROR_LIMIT_IN_PROMILS, GEN_QUALITY_COEF = 120, 0.65
MATCHING_MODE, READ_SEED_LENGTH, MIN_CHARS_PER_MISMATCH, TARGET_PG_MATCH_LENGTH = "c", 38, 3, 45
PARALLEL_PG_GENERATION_READS_COUNT_THRESHOLD = 50000             # pgrc-encoder.h; INTEGRATION.md §9
PIECE_BYTES = 64 << 20                                           # of source text handed to the divider at a time


def default_book() -> bytes:
    """a var-len DNA book in writeBook's form (VarLenDNACoder.cpp:41-52): 256 codes, '\\n' between them.  Code 0 is "A"
    (initUsing wants a single symbol there, :23-26); then the other symbols of a mapped text (C G T N and the match mark
    '%'), every pair and triple over ACGT, and the first 170 quadruples in ACGT order"""
    acgt = "ACGT"
    codes = ["A", "C", "G", "T", "N", "%"]
    for k in (2, 3, 4):
        codes += ["".join(t) for t in itertools.product(acgt, repeat=k)]
    return "\n".join(codes[:256]).encode()


# ---------------------------------------------------------------------------------------------------- compress
def _first_read_length(head: bytes, fmt: int) -> int:
    """probeReadsLength (pgrc-encoder.cpp:511-518): the length of the first read"""
    lines = head.split(b"\n")
    k = 0 if fmt == 2 else 1                                     # FASTQ, FASTA: the line behind the first header
    if len(lines) <= k:
        raise ValueError("the source holds no read")
    return len(lines[k].rstrip(b"\r"))


def _divide(div, sets, fmt: int, src: str, pair: Optional[str], rev_compl_pair: bool) -> None:
    """the two files through the divider a piece at a time, what it did not consume handed over again in front of the next
    piece (the contract of pgrc_divider_run_text: final_piece 1 where nothing follows in either file, 2 / 4 where only the
    first / the second ends here); every batch is appended to the sets on the device.  Pair files of unequal length end where
    the reference's iteration ends (pgrc_divider_last_was_terminal)."""
    with open(src, "rb") as f, open(pair if pair else os.devnull, "rb") as g:
        rest, prest, end_a, end_b = b"", b"", False, not pair
        while True:
            a = b"" if end_a else f.read(PIECE_BYTES)
            b = b"" if end_b else g.read(PIECE_BYTES)
            end_a, end_b = end_a or len(a) < PIECE_BYTES, end_b or len(b) < PIECE_BYTES
            final = 1 if end_a and end_b else (2 if end_a else 0) | (4 if end_b else 0)
            piece, ppiece = rest + a, prest + b
            _, n_records, used, pused = div.divide_text(fmt, piece, ppiece if pair else None, rev_compl_pair, final=final)
            sets.append_divider(div)
            if final == 1 or div.last_was_terminal():
                return
            if not n_records and not end_a and not end_b:
                raise ValueError("compress: a record longer than a piece of the source text")
            rest, prest = piece[used:], ppiece[pused:]


def _rule(ovl: OverlapFinder, threads_rule: int, count: int) -> None:
    """the generator the encoder picks per read set (pgrc-encoder.cpp:290, :312, :405, :430)"""
    ovl.set_rule("parallel" if threads_rule > 1 and count > PARALLEL_PG_GENERATION_READS_COUNT_THRESHOLD else "serial")


def _empty_hq_list() -> dict:
    """compressedBuild of a list without an entry: every stream empty, no offset stream, the default bases order"""
    z = np.zeros(0, np.uint8)
    return {"off": z, "rev_comp": z, "archive": {"zero_flags": z, "nonzero_cnt": z, "mis_sym": z, "bases_order": ar.EMPTY_BASES_ORDER,
                                                 "props": np.zeros(1, np.uint8), "dests": [z]}}


def compress(src: str, pair: Optional[str] = None, archive: Optional[str] = None, preserve_order: bool = False,
             threads_rule: int = 1, device: int = 0, coder: Optional[Callable] = None, book: Optional[bytes] = None,
             **expert) -> dict:
    """FASTQ, FASTA or one-read-per-line text (chosen by the first byte, as the reference does) -> a PgRC archive.

    archive: the file to write (default: src + ".pgrc").  threads_rule: the reference's -t, which only picks the overlap rule
    (INTEGRATION.md §9).  coder: archive.write_archive's plug-in; without one every stream is stored raw.  -> the archive's
    path, size and mode, and the counts of the three lists.

    Refused (NotImplementedError): PGRC_MIN_PE_MODE and the expert options at other values than the defaults; reads longer
    than 255; the ORD modes where no two reads overlap (no HQ pseudogenome); every mode but SE where there is an HQ
    pseudogenome and no read can be mapped on it (no LQ or N read at all, or a pseudogenome shorter than the seed).  A pair
    file beside one-read-per-line text is the library's to refuse."""
    archive = archive if archive is not None else src + ".pgrc"
    parts, report = compress_parts(src, pair, preserve_order, threads_rule, device, book, **expert)
    report["archive"], report["bytes"] = archive, ar.write_archive(archive, parts, coder)
    return report


def compress_parts(src: str, pair: Optional[str] = None, preserve_order: bool = False, threads_rule: int = 1, device: int = 0,
                   book: Optional[bytes] = None, **expert):
    """compress up to the file: -> (the parts archive.write_archive takes, the report compress returns)"""
    for k, v in expert.items():
        default = {"quality_error_limit_in_promils": ERROR_LIMIT_IN_PROMILS, "generator_overlap_threshold": GEN_QUALITY_COEF,
                   "read_seed_length": READ_SEED_LENGTH, "min_chars_per_mismatch": MIN_CHARS_PER_MISMATCH,
                   "target_pg_match_length": TARGET_PG_MATCH_LENGTH, "ignore_pair_order": False}
        if k not in default:
            raise TypeError(f"compress: unknown option {k}")
        if v != default[k]:
            raise NotImplementedError(f"compress: {k} = {v!r} is out of scope (PGRC_MIN_PE_MODE and the expert options -q -g -s -M -p "
                                      "are offered at their defaults only)")
    paired = pair is not None
    mode = (ar.PGRC_ORD_PE_MODE if paired else ar.PGRC_ORD_SE_MODE) if preserve_order else (ar.PGRC_PE_MODE if paired else ar.PGRC_SE_MODE)
    with open(src, "rb") as f:
        head = f.read(1 << 16)
    fmt = reads_text_format(head[:1])
    L = _first_read_length(head, fmt)
    if not 0 < L <= 255:
        raise NotImplementedError(f"compress: reads of {L} symbols (1 to 255 are supported)")
    rev_compl_pair_file = paired                                 # pgrc-encoder.cpp:49-54
    held = []

    def keep(x):
        held.append(x)
        return x
    try:
        # 1. the division (runQualityBasedDivision, :254-262) and 2. the sets on the device
        #    (FASTA and one-read-per-line text carry no qualities to divide by: include/pgrc_reads.h)
        error_limit = ERROR_LIMIT_IN_PROMILS / 1000.0 if fmt == _lib.reads_format("fastq") else 1.0
        div = keep(DividedPCLReadsSets(L, error_limit, True, True, False, device=device))
        sets = keep(DividedReadsSets(L, True, False, device=device))
        _divide(div, sets, fmt, src, pair, rev_compl_pair_file)
        sets.finish()
        T = sets.info()["reads_total_count"]
        if T == 0 or (paired and T % 2):
            raise ValueError(f"compress: {T} reads" + (" in two files of unequal length" if paired else ""))
        # 3. the generator-based division (runPgGeneratorBasedReadsDivision, :286-296)
        ovl = keep(OverlapFinder(device=device))
        if sets.info()["count"][0]:
            _rule(ovl, threads_rule, sets.info()["count"][0])
            sets.overlap("hq", ovl, GEN_QUALITY_COEF)
            sets.move_by_overlap(ovl)
        # 4. the HQ pseudogenome (runHQPgGeneration, :309-323)
        n_hq = sets.info()["count"][0]
        asm = {w: keep(PgAssembler(device=device)) for w in ar.LISTS}
        lists = {w: keep(ReadsList(device)) for w in ar.LISTS}
        if n_hq:
            _rule(ovl, threads_rule, n_hq)
            sets.overlap("hq", ovl)
            lists["hq"].from_overlap(ovl, asm["hq"], sets, "hq")
        hq_len = asm["hq"].pg_len if n_hq else 0
        # 5. the LQ and N reads on the HQ pseudogenome (runMappingLQReadsOnHQPg, :342-374) and 6./7. the export and its
        #    archive form (mapReadsIntoPg's exportMatchesInPgOrder / InOriginalOrder and compressedBuild)
        prm = MatchParams()
        if lib.pgrc_match_derive_params(L, READ_SEED_LENGTH, MIN_CHARS_PER_MISMATCH, MATCHING_MODE.encode(), C.byref(prm)):
            raise PgrcMatchError(3, "bad matching parameters")
        parts = {"mode": mode, "read_length": L, "separate_n": True, "rev_compl_pair_file": rev_compl_pair_file,
                 "compression_level": ar.CODER_LEVEL_NORMAL, "name": "pgrc_amd"}
        ctx, read_org, hq_part = None, None, None
        n_rest = sets.info()["count"][1] + sets.info()["count"][2]
        if n_hq and n_rest and hq_len >= prm.seed_len:
            ctx = keep(MatchContext(L, prm.seed_len, prm.max_mismatches, prm.min_mismatches, prm.mode.decode(), device=device))
            ctx.set_pg_packed_device(asm["hq"].packed_device(), hq_len)
            sets.to_matcher(ctx)
            ctx.init_results()
            ctx.run(True)
        if n_hq and ctx is not None:
            if preserve_order:
                # (the positions of stage 9 want the matcher's reads under the indexes they had when it ran: INTEGRATION.md §13)
                read_org = np.concatenate([sets.get_mapping("lq")[:-1], sets.get_mapping("n")[:-1]])
                exp = keep(ReadsList(device))
                exp.export_original_order(ctx, T, None, sets, paired, rev_compl_pair_file, True)
                a = exp.archive_encode_ord()
            else:
                lists["hq"].export_pg_order(ctx, None, None, sets, rev_compl_pair_file, True)
                a = lists["hq"].archive_encode(False, False)
            hq_part = {"n_entries": a["n_entries"], "off": a["off"], "rev_comp": a["rev_comp"], "archive": a["archive"]}
            sets.remove_matched(ctx)
        elif n_hq:
            # no read to map, or a pseudogenome shorter than the seed: mapReadsIntoPg exports the list as it is, every entry
            # forward and without a mismatch.  The one place where flags of the reads' number are made on the host.
            if mode != ar.PGRC_SE_MODE:
                raise NotImplementedError(f"compress: {ar.MODE_NAMES[mode]} mode where no read can be mapped on the HQ pseudogenome "
                                          f"({n_rest} reads beside it, {hq_len} symbols): only the SE mode writes that case")
            hq_part = dict(_empty_hq_list(), n_entries=n_hq, off=lists["hq"].archive_encode(False, False)["off"], rev_comp=np.zeros(n_hq, np.uint8))
            hq_part["archive"]["zero_flags"] = np.ones(n_hq, np.uint8)
        else:
            hq_part = dict(_empty_hq_list(), n_entries=0)
        hq_part["pg_length"] = hq_len
        parts["hq"] = hq_part
        # 8. the LQ and N pseudogenomes (runLQPgGeneration, runNPgGeneration, :402-439)
        count = sets.info()["count"]
        for w, k in (("lq", 1), ("n", 2)):
            if count[k]:
                _rule(ovl, threads_rule, count[k])
                sets.overlap(w, ovl)
                lists[w].from_overlap(ovl, asm[w], sets, w)
                off = None if preserve_order else lists[w].archive_encode(False, False)["off"]
                parts[w] = {"n_entries": count[k], "pg_length": asm[w].pg_len, "off": off}
            else:
                lists[w] = None
                parts[w] = {"n_entries": 0, "pg_length": 0, "off": np.zeros(0, np.uint8)}
        lq_len, n_len = parts["lq"]["pg_length"], parts["n"]["pg_length"]
        hq_list = lists["hq"] if n_hq else None
        # 9. the order (compressReadsPgPositions / compressReadsOrder, :209-227)
        if preserve_order:
            if hq_list is None:
                raise NotImplementedError(f"compress: {ar.MODE_NAMES[mode]} mode without an HQ pseudogenome (no two reads overlap): "
                                          "the SE and PE modes write that case")
            width = 4 if hq_len + lq_len + n_len <= 0xFFFFFFFF else 8
            args = (T, width, lists["lq"], lists["n"], hq_len, lq_len, ctx, read_org)
            parts["order"] = hq_list.pair_positions(*args) if paired else {"positions": hq_list.positions(*args)}
        elif paired:
            parts["order"] = ReadsList.pair_order([hq_list, lists["lq"], lists["n"]], PGRC_PAIRORDER_FILE_FLAGS)
        # 10.-12. the pseudogenomes in each other (SimplePgMatcher::matchPgsInPg, SimplePgMatcher.cpp:175-257)
        book = default_book() if book is None else bytes(book).rstrip(b"\0")
        vl = keep(VarLenDNACoder(book + b"\0", device=device))
        texts = [(asm[w].text_device() if parts[w]["pg_length"] else (0, 0)) for w in ar.LISTS]
        g = {"map_off": [b"", b"", b""], "map_len": [b"", b"", b""]}
        frugal_min = bytes([TARGET_PG_MATCH_LENGTH])             # writeUIntByteFrugal(minMatchLength) (:92): one byte below 128
        if hq_len >= TARGET_PG_MATCH_LENGTH:
            tm = keep(CopMEMMatcher(None, TARGET_PG_MATCH_LENGTH, device=device))
            tm.setSrcDevice(*texts[0])
            resident = texts[1][1] > 0                           # (pgrc_mem_encode_mapped wants the HQ and the LQ slot filled)
            host = [np.zeros(0, np.uint8)] * 3
            for p in (1, 2, 0):                                  # LQ, N, HQ (:185-205)
                ptr, n = texts[p]
                if not n:                                        # an empty text: no match, no offset, the lengths' first byte (:89-143)
                    g["map_len"][p] = frugal_min
                    continue
                found = tm.matchTextsDevice(ptr, n, p == 0, True)
                if resident:
                    _, g["map_off"][p], g["map_len"][p], _ = tm.markAndRemoveExactMatchesResident(found, p)
                else:
                    mapped, g["map_off"][p], g["map_len"][p], _ = tm.markAndRemoveExactMatches(found)
                    host[p] = mapped.copy()
            if resident:
                coded, lens = tm.encodeMapped(vl)
            else:
                coded, lens = vl.encode(host), tuple(int(h.size) for h in host)
        else:                                                    # no matcher (:16-17, :72-76): the texts as they are, no mapping stream
            coded, lens = vl.encode([(ptr, n) for ptr, n in texts]), tuple(n for _, n in texts)
        g["mapped_lens"] = lens
        g["mapped"] = ar.VarLenCoded(book, coded, sum(lens))
        parts["pgs"] = g
        return parts, {"mode": mode, "read_length": L, "reads": T,
                       "counts": tuple(parts[w]["n_entries"] for w in ar.LISTS), "pg_lengths": (hq_len, lq_len, n_len), "mapped_lengths": tuple(lens)}
    finally:
        for x in reversed(held):
            x.close()


# ---------------------------------------------------------------------------------------------------- decompress
def load(archive: str, device: int = 0, decoder: Optional[Callable] = None):
    """the archive as a decode job: -> (PgRCDecoder with the text, the three lists and the order set, the archive's parts).
    The caller closes the decoder.  What loadAllPgs does (pgrc-decoder.cpp:727-827), the pseudogenomes restored, the lists
    rebuilt and the order decoded on the device."""
    parts = ar.read_archive(archive, decoder)
    mode = parts["mode"]
    L = parts["read_length"]
    hq, lq, nl, g = parts["hq"], parts["lq"], parts["n"], parts["pgs"]
    dec = PgRCDecoder(L, device=device)
    vl = None
    try:
        mapped = g["mapped"]
        if not any(len(x) for x in g["map_len"]):                # written without a matcher: the texts are the mapped texts
            if isinstance(mapped, ar.VarLenCoded):
                vl = VarLenDNACoder(mapped.book + b"\0", device=device)
                mapped = vl.decode(mapped.payload, mapped.dest_len) if mapped.dest_len else np.zeros(0, np.uint8)
            dec.set_text(np.frombuffer(bytes(mapped), dtype=np.uint8) if isinstance(mapped, bytes) else mapped)
        elif isinstance(mapped, ar.VarLenCoded):
            vl = VarLenDNACoder(mapped.book + b"\0", device=device)
            dec.set_mapped_text_coded(vl, mapped.payload, g["mapped_lens"], hq["pg_length"], g["map_off"], g["map_len"], True)
        else:
            dec.restoreMatchedPgs(mapped, g["mapped_lens"], hq["pg_length"], g["map_off"], g["map_len"], True)
        got = dec.text_lengths() if any(len(x) for x in g["map_len"]) else None
        want = (hq["pg_length"], lq["pg_length"], nl["pg_length"])
        if got is not None and tuple(got) != want:
            raise ar.ArchiveError(f"the restored pseudogenomes have the lengths {tuple(got)}, their properties say {want}")
        dec.add_list_archive(hq["n_entries"], hq["archive"], 0, off=hq["off"], rev_comp=hq["rev_comp"])
        dec.add_list(lq["n_entries"], want[0], off=lq["off"])
        dec.add_list(nl["n_entries"], want[0] + want[1], off=nl["off"])
        o, rc = parts["order"], parts["rev_compl_pair_file"]
        if mode == ar.PGRC_SE_MODE:
            dec.set_order(PGRC_DECODE_SE)
        elif mode == ar.PGRC_PE_MODE:
            dec.set_order_pair_order_streams(o, rc)
        elif mode == ar.PGRC_ORD_SE_MODE:
            dec.set_order_positions(o["positions"], rc)
        else:
            dec.set_order_pair_streams(o, rc)
    except BaseException:
        dec.close()
        raise
    finally:
        if vl is not None:
            vl.close()
    return dec, parts


def decompress(archive: str, out_prefix: Optional[str] = None, device: int = 0, decoder: Optional[Callable] = None):
    """a PgRC archive -> its reads: one (n, L+1) uint8 array per output file (every row L symbols and '\\n'), or, with
    out_prefix, the files the reference names (<out_prefix>_out, or _out_1 and _out_2; pgrc-decoder.cpp:150, :259) and
    their paths.  decoder: archive.read_archive's plug-in for the streams that are not stored raw."""
    dec, parts = load(archive, device, decoder)
    try:
        files = 2 if parts["mode"] in ar.PAIRED_MODES else 1
        if out_prefix is None:
            return tuple(dec.rows(p) for p in range(files))
        names = [out_prefix + "_out"] if files == 1 else [out_prefix + "_out_1", out_prefix + "_out_2"]
        step = max(1, (64 << 20) // (parts["read_length"] + 1))
        for p, name in enumerate(names):
            with open(name, "wb") as f:
                n = dec.row_count(p)
                for first in range(0, n, step):
                    f.write(dec.rows(p, first, min(step, n - first)).tobytes())
        return tuple(names)
    finally:
        dec.close()
