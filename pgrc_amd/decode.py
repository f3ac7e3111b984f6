"""Host-side mirror of the reference decoder's read rebuild (pgrc/pgrc-decoder.cpp) over include/pgrc_decode.h: the reads
are rebuilt from the pseudogenomes and their reads lists on the MI355X.  No compute here.

The class's methods are named after the reference's three writers; each returns the rows of every output file as
uint8 arrays of shape (n, L+1), a row being L symbols and '\\n'."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import ExportStreams, ListArchiveStreams, ListArchiveTiming, PairOrderDecodeTiming, PgrcMatchError, lib

_P = C.c_void_p

PGRC_DECODE_SE, PGRC_DECODE_PE, PGRC_DECODE_ORD = 0, 1, 2


class DecodeList(C.Structure):      # pgrc_decode_list
    _fields_ = [("struct_size", C.c_uint32), ("text_base", C.c_uint64), ("n_entries", C.c_uint64), ("off", _P),
                ("off_width", C.c_uint32), ("pos", _P), ("rev_comp", _P), ("mis_cnt", _P), ("mis_sym", _P),
                ("mis_off", _P), ("mis_off_width", C.c_uint32), ("mis_off_rev_coded", C.c_int32),
                ("mis_sym_form", C.c_int32), ("bases_order", C.c_char_p)]


class DecodeOrder(C.Structure):     # pgrc_decode_order
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("n_total", C.c_uint64), ("rl_idx_order", _P),
                ("org_idx_to_pos", _P), ("paired", C.c_int32), ("rev_compl_pair_file", C.c_int32)]


class DecodeTiming(C.Structure):    # pgrc_decode_timing
    _fields_ = [("ms_text", C.c_float), ("ms_lists_device", C.c_float), ("ms_order_device", C.c_float),
                ("ms_rows_device", C.c_float), ("ms_rows", C.c_float), ("rows_bytes", C.c_uint64)]


class DecodeMapped(C.Structure):    # pgrc_decode_mapped
    _fields_ = [("struct_size", C.c_uint32), ("mapped", _P), ("mapped_len", C.c_uint64 * 3), ("org_hq_len", C.c_uint64),
                ("map_off", _P * 3), ("map_off_bytes", C.c_uint64 * 3), ("map_len", _P * 3),
                ("map_len_bytes", C.c_uint64 * 3), ("rev_compl", C.c_int32)]


class RestoreTiming(C.Structure):   # pgrc_decode_restore_timing
    _fields_ = [("struct_size", C.c_uint32), ("ms_upload", C.c_float), ("ms_parse_device", C.c_float),
                ("ms_literals_device", C.c_float), ("ms_matches_device", C.c_float), ("ms_call", C.c_float),
                ("passes", C.c_uint32), ("marks", C.c_uint64 * 3), ("matched", C.c_uint64 * 3)]


class PairPosStreams(C.Structure):  # pgrc_pairpos_streams
    _fields_ = [("struct_size", C.c_uint32), ("pos_width", C.c_uint32), ("n_total", C.c_uint64), ("base_pos", _P),
                ("off16_flag", _P), ("off_base_first", _P), ("off_value", _P), ("delta16_flag", _P),
                ("delta_base_first", _P), ("delta_value", _P), ("not_base_pos", _P), ("n_off16", C.c_uint64),
                ("n_delta_flag", C.c_uint64), ("n_delta16", C.c_uint64), ("n_not_base", C.c_uint64)]


class PairPosTiming(C.Structure):   # pgrc_pairpos_timing
    _fields_ = [("struct_size", C.c_uint32), ("encode", C.c_int32), ("ms_upload", C.c_float),
                ("ms_sort_device", C.c_float), ("ms_scan_device", C.c_float), ("ms_scatter_device", C.c_float),
                ("ms_download", C.c_float), ("ms_call", C.c_float), ("bytes_up", C.c_uint64),
                ("bytes_down", C.c_uint64), ("n_near", C.c_uint64), ("n_delta", C.c_uint64), ("n_full", C.c_uint64)]


PGRC_PAIRORDER_IGNORE, PGRC_PAIRORDER_FILE_FLAGS, PGRC_PAIRORDER_COMPLETE, PGRC_PAIRORDER_COMPLETE_SINGLE_FILE = 0, 1, 2, 3


class PairOrderStreams(C.Structure):    # pgrc_pairorder_streams
    _fields_ = [("struct_size", C.c_uint32), ("form", C.c_int32), ("n_total", C.c_uint64), ("off8_flag", _P),
                ("off_value", _P), ("delta8_flag", _P), ("delta_value", _P), ("full_offset", _P),
                ("pair_base_org_idx", _P), ("off_base_file_flag", _P), ("nonoff_base_file_flag", _P), ("rev", _P),
                ("n_off8", C.c_uint64), ("n_delta_flag", C.c_uint64), ("n_delta8", C.c_uint64), ("n_full", C.c_uint64)]


class PairOrderTiming(C.Structure):     # pgrc_pairorder_timing
    _fields_ = [("struct_size", C.c_uint32), ("form", C.c_int32), ("ms_upload", C.c_float),
                ("ms_inverse_device", C.c_float), ("ms_scatter_device", C.c_float), ("ms_scan_device", C.c_float),
                ("ms_compact_device", C.c_float),
                ("ms_download", C.c_float), ("ms_call", C.c_float), ("bytes_up", C.c_uint64),
                ("bytes_down", C.c_uint64), ("n_near", C.c_uint64), ("n_delta", C.c_uint64), ("n_full", C.c_uint64)]


# include/pgrc_decode.h (kept apart from _lib._PROTOS, which mirrors pgrc_match.h / pgrc_mem.h / pgrc_reads.h)
DECODE_PROTOS = [
    ("pgrc_decode_create", C.c_int, [C.c_uint32, C.c_int32, C.POINTER(_P)]),
    ("pgrc_decode_destroy", None, [_P]),
    ("pgrc_decode_last_error", C.c_char_p, [_P]),
    ("pgrc_decode_set_text", C.c_int, [_P, _P, C.c_uint64]),
    ("pgrc_decode_add_list", C.c_int, [_P, C.POINTER(DecodeList)]),
    ("pgrc_decode_set_order", C.c_int, [_P, C.POINTER(DecodeOrder)]),
    ("pgrc_decode_row_count", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("pgrc_decode_rows", C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_uint64, _P]),
    ("pgrc_decode_rows_device", C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_uint64, _P]),
    ("pgrc_decode_get_timing", C.c_int, [_P, C.POINTER(DecodeTiming)]),
    ("pgrc_decode_set_mapped_text", C.c_int, [_P, C.POINTER(DecodeMapped)]),
    ("pgrc_decode_set_mapped_text_coded", C.c_int, [_P, C.POINTER(DecodeMapped), _P, _P, C.c_uint64]),
    ("pgrc_decode_text_lengths", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("pgrc_decode_get_text", C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    ("pgrc_decode_get_restore_timing", C.c_int, [_P, C.POINTER(RestoreTiming)]),
    ("pgrc_pairpos_encode", C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.POINTER(PairPosStreams)]),
    ("pgrc_pairpos_free", None, [C.POINTER(PairPosStreams)]),
    ("pgrc_pairpos_decode", C.c_int, [_P, C.POINTER(PairPosStreams), _P]),
    ("pgrc_decode_set_order_pair_streams", C.c_int, [_P, C.POINTER(PairPosStreams), C.c_int32]),
    ("pgrc_decode_set_order_positions", C.c_int, [_P, _P, C.c_uint32, C.c_uint64, C.c_int32]),
    ("pgrc_pairpos_get_timing", C.c_int, [_P, C.POINTER(PairPosTiming)]),
    ("pgrc_pairorder_encode", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64), C.c_int32, C.POINTER(PairOrderStreams)]),
    ("pgrc_pairorder_free", None, [C.POINTER(PairOrderStreams)]),
    ("pgrc_pairorder_get_timing", C.c_int, [_P, C.POINTER(PairOrderTiming)]),
    ("pgrc_pairorder_decode", C.c_int, [_P, C.POINTER(PairOrderStreams), _P]),
    ("pgrc_decode_set_order_pair_order_streams", C.c_int, [_P, C.POINTER(PairOrderStreams), C.c_int32]),
    ("pgrc_pairorder_get_decode_timing", C.c_int, [_P, C.POINTER(PairOrderDecodeTiming)]),
    ("pgrc_list_archive_encode", C.c_int, [_P, C.POINTER(ExportStreams), C.c_int32, C.POINTER(ListArchiveStreams)]),
    ("pgrc_list_archive_free", None, [C.POINTER(ListArchiveStreams)]),
    ("pgrc_decode_add_list_archive", C.c_int, [_P, C.POINTER(DecodeList), C.POINTER(ListArchiveStreams)]),
    ("pgrc_list_archive_get_timing", C.c_int, [_P, C.POINTER(ListArchiveTiming)]),
]
for _name, _res, _args in DECODE_PROTOS:
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


def _bytes(a) -> np.ndarray:
    """bytes, bytearray, str or an array as a contiguous uint8 array (None: empty)"""
    if a is None:
        return np.zeros(0, np.uint8)
    if isinstance(a, str):
        a = a.encode("latin-1")
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# the eight streams of the pair-position coding, in the archive's order, with their element types (the two position
# streams are uint32 or uint64 by pos_width)
PAIRPOS_STREAMS = (("base_pos", None), ("off16_flag", np.uint8), ("off_base_first", np.uint8), ("off_value", np.uint16),
                   ("delta16_flag", np.uint8), ("delta_base_first", np.uint8), ("delta_value", np.int16),
                   ("not_base_pos", None))


def _pairpos_struct(streams: dict):
    """the dict compressReadsPgPositions returns (stream name -> array, plus n_total and pos_width) as a
    pgrc_pairpos_streams; the counts are the arrays' sizes.  -> (struct, the arrays it points into)"""
    w = int(streams["pos_width"])
    s = PairPosStreams()
    s.struct_size = C.sizeof(PairPosStreams)
    s.pos_width = w
    s.n_total = int(streams["n_total"])
    keep = []
    for name, dt in PAIRPOS_STREAMS:
        a = np.ascontiguousarray(streams[name], dtype=dt if dt is not None else (np.uint64 if w == 8 else np.uint32))
        keep.append(a)
        setattr(s, name, _ptr(a) if a.size else None)
    s.n_off16 = int(streams.get("n_off16", keep[2].size))
    s.n_delta_flag = int(streams.get("n_delta_flag", keep[4].size))
    s.n_delta16 = int(streams.get("n_delta16", keep[5].size))
    s.n_not_base = int(streams.get("n_not_base", keep[7].size))
    return s, keep


# the streams of the pair-order coding in the struct's order, with their element types
PAIRORDER_STREAMS = (("off8_flag", np.uint8), ("off_value", np.uint8), ("delta8_flag", np.uint8), ("delta_value", np.int8),
                     ("full_offset", np.uint32), ("pair_base_org_idx", np.uint32), ("off_base_file_flag", np.uint8),
                     ("nonoff_base_file_flag", np.uint8), ("rev", np.uint32))


PGRC_PAIRORDER_DECODE_BATCH = 16384  # entries of one batch of the pair-order landing (include/pgrc_decode.h)


def _pairorder_struct(streams: dict):
    """the dict compressReadsOrder returns (stream name -> array, plus n_total and form) as a pgrc_pairorder_streams: the
    streams the dict does not hold stay NULL; the counts are the arrays' sizes unless the dict names them (n_off8,
    n_delta_flag, n_delta8, n_full).  -> (struct, the arrays it points into)"""
    s = PairOrderStreams()
    s.struct_size = C.sizeof(PairOrderStreams)
    s.form = int(streams["form"])
    s.n_total = int(streams["n_total"])
    keep = {}
    for name, dt in PAIRORDER_STREAMS:
        if streams.get(name) is None:
            continue
        a = keep[name] = np.ascontiguousarray(streams[name], dtype=dt)
        setattr(s, name, _ptr(a) if a.size else None)

    def size(name):
        return keep[name].size if name in keep else 0
    s.n_off8 = int(streams.get("n_off8", size("off_value")))
    s.n_delta_flag = int(streams.get("n_delta_flag", size("delta8_flag")))
    s.n_delta8 = int(streams.get("n_delta8", size("delta_value")))
    s.n_full = int(streams.get("n_full", size("full_offset")))
    return s, keep


PGRC_LIST_ARCHIVE_TILE = 8192       # entries of one tile of the split (include/pgrc_decode.h)


def _u8ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.size else None


def _export_struct(mis_cnt, mis_sym, mis_rev_off):
    """the three mismatch streams of a pgrc_export_streams (the other streams stay NULL) -> (struct, the arrays it points into)"""
    keep = [_bytes(mis_cnt), _bytes(mis_sym), np.ascontiguousarray(mis_rev_off)]
    x = ExportStreams()
    x.n_entries, x.n_mismatches, x.off_width = keep[0].size, keep[1].size, keep[2].dtype.itemsize
    keep[2] = keep[2].view(np.uint8).reshape(-1)
    x.mis_cnt, x.mis_sym, x.mis_rev_off = _u8ptr(keep[0]), _u8ptr(keep[1]), _u8ptr(keep[2])
    return x, keep


def _list_archive_struct(st: dict):
    """the dict list_archive_encode returns as a pgrc_list_archive_streams; the counts are the arrays' sizes unless the dict
    names them (n_entries, n_mismatches, n_nonzero, n_dests, props_len, dest_len).  -> (struct, the arrays it points into)"""
    s = ListArchiveStreams()
    s.struct_size = C.sizeof(ListArchiveStreams)
    keep = {k: _bytes(st[k]) for k in ("zero_flags", "nonzero_cnt", "mis_sym", "props")}
    for k, a in keep.items():
        setattr(s, k, _ptr(a) if a.size else None)
    s.n_entries = int(st.get("n_entries", keep["zero_flags"].size))
    s.n_mismatches = int(st.get("n_mismatches", keep["mis_sym"].size))
    s.n_nonzero = int(st.get("n_nonzero", keep["nonzero_cnt"].size))
    s.props_len = int(st.get("props_len", keep["props"].size))
    s.bases_order = bytes(st["bases_order"])
    dests = [_bytes(a) for a in st["dests"]]
    s.n_dests = int(st.get("n_dests", len(dests) - 1))
    lens = st.get("dest_len", [a.size for a in dests])
    for c in range(1, min(len(dests), 255)):
        s.dest[c] = dests[c].ctypes.data if dests[c].size else None
        s.dest_len[c] = int(lens[c])
    return s, (keep, dests)


def _pairpos_dict(s) -> dict:
    """the eight streams of a filled pgrc_pairpos_streams by name (copies), n_total and pos_width"""
    T, pos_width = int(s.n_total), int(s.pos_width)
    cnt = {"base_pos": T // 2, "off16_flag": T // 2, "off_base_first": s.n_off16,
           "off_value": s.n_off16, "delta16_flag": s.n_delta_flag, "delta_base_first": s.n_delta16,
           "delta_value": s.n_delta16, "not_base_pos": s.n_not_base}
    out = {"n_total": T, "pos_width": pos_width}
    for name, dt in PAIRPOS_STREAMS:
        dt = np.dtype(dt if dt is not None else (np.uint64 if pos_width == 8 else np.uint32))
        n = int(cnt[name])
        out[name] = (np.frombuffer((C.c_uint8 * (n * dt.itemsize)).from_address(getattr(s, name)), dtype=dt).copy()
                     if n else np.zeros(0, dt))
    return out


def _pairorder_dict(s) -> dict:
    """the streams a filled pgrc_pairorder_streams holds for its form by name (copies), n_total and form"""
    T, form = int(s.n_total), int(s.form)
    coded = form != PGRC_PAIRORDER_COMPLETE_SINGLE_FILE
    cnt = {"off8_flag": T // 2 if coded else 0, "off_value": s.n_off8, "delta8_flag": s.n_delta_flag,
           "delta_value": s.n_delta8, "full_offset": s.n_full, "pair_base_org_idx": T // 2,
           "off_base_file_flag": s.n_off8, "nonoff_base_file_flag": s.n_delta_flag, "rev": T}
    present = (PAIRORDER_STREAMS[:5] if coded else ()) + {PGRC_PAIRORDER_IGNORE: (), PGRC_PAIRORDER_FILE_FLAGS: PAIRORDER_STREAMS[6:8],
                                                           PGRC_PAIRORDER_COMPLETE: PAIRORDER_STREAMS[5:6]}.get(form, PAIRORDER_STREAMS[8:])
    out = {"n_total": T, "form": form}
    for name, dt in present:
        dt = np.dtype(dt)
        n = int(cnt[name])
        out[name] = (np.frombuffer((C.c_uint8 * (n * dt.itemsize)).from_address(getattr(s, name)), dtype=dt).copy()
                     if n else np.zeros(0, dt))
    return out


def _list_archive_dict(s, block=None) -> dict:
    """a filled pgrc_list_archive_streams as list_archive_encode returns it (copies); block: where its one block starts"""
    def take(p, n):
        return np.frombuffer((C.c_uint8 * n).from_address(p), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)
    block = s.block if block is None else block
    return {"n_entries": int(s.n_entries), "n_mismatches": int(s.n_mismatches), "n_nonzero": int(s.n_nonzero),
            "zero_flags": take(s.zero_flags, int(s.n_entries)), "nonzero_cnt": take(s.nonzero_cnt, int(s.n_nonzero)),
            "mis_sym": take(s.mis_sym, int(s.n_mismatches)), "bases_order": bytes(s.bases_order[:5]),
            "props": take(s.props, int(s.props_len)),
            "dests": [np.zeros(0, np.uint8)] + [take(s.dest[c], int(s.dest_len[c])) for c in range(1, int(s.n_dests) + 1)],
            "one_block": all(s.dest[c] is None or block <= s.dest[c] < s.props for c in range(1, int(s.n_dests) + 1))}


class PgRCDecoder:
    """The reads of a decoded archive, rebuilt on the device: the joined text HQ | LQ | N, the three reads lists, then
    one of the three writers."""

    def __init__(self, read_length: int, device: int = -1):
        self._h = _P()
        rc = lib.pgrc_decode_create(int(read_length), int(device), C.byref(self._h))
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_decode_last_error(None) or b"").decode())
        self.readLength = int(read_length)
        self._text_len = 0

    def _ck(self, rc: int) -> None:
        if rc:
            raise PgrcMatchError(rc, (lib.pgrc_decode_last_error(self._h) or b"").decode())

    def set_text(self, joined) -> None:
        """the joined pseudogenome text (bytes or uint8 array); copied to the device"""
        t = np.frombuffer(joined, dtype=np.uint8) if isinstance(joined, (bytes, bytearray)) else _arr(joined, np.uint8)
        self._text_len = 0
        self._ck(lib.pgrc_decode_set_text(self._h, _ptr(t), t.size))
        self._text_len = t.size

    def restoreMatchedPgs(self, mapped, mapped_lens, org_hq_len: int, map_off, map_len, rev_compl: bool = True) -> None:
        """SimplePgMatcher::restoreMatchedPgs (SimplePgMatcher.cpp:259-351) on the device: `mapped` is the joined mapped
        text HQ | LQ | N (comboPgMapped) with the part lengths `mapped_lens`; map_off and map_len hold the three parts'
        offsets and byte-frugal lengths streams (None or empty for an absent part).  Installs the restored joined text
        as set_text would; the lists and the order are dropped."""
        t = _bytes(mapped)
        lens = [int(x) for x in mapped_lens]
        assert len(lens) == 3 and sum(lens) == t.size and len(map_off) == 3 and len(map_len) == 3
        offs = [_bytes(x) for x in map_off]
        lns = [_bytes(x) for x in map_len]
        a = DecodeMapped()
        a.struct_size = C.sizeof(DecodeMapped)
        a.mapped = _ptr(t)
        a.org_hq_len = int(org_hq_len)
        a.rev_compl = int(bool(rev_compl))
        for p in range(3):
            a.mapped_len[p] = lens[p]
            a.map_off[p], a.map_off_bytes[p] = _ptr(offs[p]), offs[p].size
            a.map_len[p], a.map_len_bytes[p] = _ptr(lns[p]), lns[p].size
        self._text_len = 0
        self._ck(lib.pgrc_decode_set_mapped_text(self._h, C.byref(a)))
        self._text_len = sum(self.text_lengths())

    def set_mapped_text_coded(self, coder, coded, mapped_lens, org_hq_len: int, map_off, map_len, rev_compl: bool = True) -> None:
        """restoreMatchedPgs with the joined mapped text still coded: `coded` is the payload of VarLenDNACoder::Compress,
        `coder` the pgrc_amd.VarLenDNACoder made from its book.  The coded bytes go up and are decoded on the device."""
        t = _bytes(coded)
        lens = [int(x) for x in mapped_lens]
        assert len(lens) == 3 and len(map_off) == 3 and len(map_len) == 3
        offs = [_bytes(x) for x in map_off]
        lns = [_bytes(x) for x in map_len]
        a = DecodeMapped()
        a.struct_size = C.sizeof(DecodeMapped)
        a.mapped = None
        a.org_hq_len = int(org_hq_len)
        a.rev_compl = int(bool(rev_compl))
        for p in range(3):
            a.mapped_len[p] = lens[p]
            a.map_off[p], a.map_off_bytes[p] = _ptr(offs[p]), offs[p].size
            a.map_len[p], a.map_len_bytes[p] = _ptr(lns[p]), lns[p].size
        self._text_len = 0
        self._ck(lib.pgrc_decode_set_mapped_text_coded(self._h, C.byref(a), coder._h, _ptr(t) if t.size else None, t.size))
        self._text_len = sum(self.text_lengths())

    def text_lengths(self) -> tuple:
        """(HQ, LQ, N) lengths of the restored text: the lists' text_base are 0, HQ and HQ + LQ"""
        v = (C.c_uint64 * 3)()
        self._ck(lib.pgrc_decode_text_lengths(self._h, v))
        return tuple(int(x) for x in v)

    def text(self, first: int = 0, n: int | None = None, out=None) -> np.ndarray:
        """bytes [first, first+n) of the installed joined text as uint8 (into `out` if given)"""
        if n is None:
            n = self._text_len - first
        if out is None:
            out = np.empty(n, dtype=np.uint8)
        assert out.flags.c_contiguous and out.nbytes == n
        self._ck(lib.pgrc_decode_get_text(self._h, int(first), int(n), out.ctypes.data_as(_P)))
        return out

    def restore_timing(self) -> dict:
        t = RestoreTiming()
        t.struct_size = C.sizeof(RestoreTiming)
        self._ck(lib.pgrc_decode_get_restore_timing(self._h, C.byref(t)))
        d = {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}
        d["marks"], d["matched"] = list(t.marks), list(t.matched)
        return d

    def add_list(self, n_entries: int, text_base: int = 0, off=None, pos=None, rev_comp=None, mis_cnt=None, mis_sym=None,
                 mis_off=None, mis_off_rev_coded: bool = True, mis_sym_form: int = 0, bases_order=None) -> None:
        """one reads list (HQ, LQ, N in that order).  off: offset deltas as uint8 or uint16 (the width follows the dtype);
        pos: absolute positions in the list's text instead; mis_off: uint8 or uint16 offsets (rev-coded by default)."""
        a = DecodeList()
        a.struct_size = C.sizeof(DecodeList)
        a.text_base = int(text_base)
        a.n_entries = int(n_entries)
        keep = []
        if off is not None:
            off = np.ascontiguousarray(off)
            assert off.dtype in (np.uint8, np.uint16) and off.size == n_entries
            a.off, a.off_width = _ptr(off), off.dtype.itemsize
            keep.append(off)
        if pos is not None:
            pos = _arr(pos, np.uint64)
            a.pos = _ptr(pos)
            keep.append(pos)
        if rev_comp is not None:
            rev_comp = _arr(rev_comp, np.uint8)
            a.rev_comp = _ptr(rev_comp)
            keep.append(rev_comp)
        if mis_cnt is not None:
            mis_cnt = _arr(mis_cnt, np.uint8)
            mis_sym = _arr(mis_sym, np.uint8)
            mis_off = np.ascontiguousarray(mis_off)
            assert mis_off.dtype in (np.uint8, np.uint16)
            a.mis_cnt, a.mis_sym, a.mis_off = _ptr(mis_cnt), _ptr(mis_sym), _ptr(mis_off)
            a.mis_off_width = mis_off.dtype.itemsize
            keep += [mis_cnt, mis_sym, mis_off]
        a.mis_off_rev_coded = int(bool(mis_off_rev_coded))
        a.mis_sym_form = int(mis_sym_form)
        a.bases_order = None if bases_order is None else (bases_order.encode() if isinstance(bases_order, str) else bytes(bases_order))
        self._ck(lib.pgrc_decode_add_list(self._h, C.byref(a)))

    def set_order(self, mode: int, n_total: int = 0, rl_idx_order=None, org_idx_to_pos=None, paired: bool = False,
                  rev_compl_pair_file: bool = False) -> None:
        o = DecodeOrder()
        o.struct_size = C.sizeof(DecodeOrder)
        o.mode = int(mode)
        o.n_total = int(n_total)
        ro = _arr(rl_idx_order, np.uint32)
        op = _arr(org_idx_to_pos, np.uint64)
        o.rl_idx_order, o.org_idx_to_pos = _ptr(ro), _ptr(op)
        o.paired = int(bool(paired))
        o.rev_compl_pair_file = int(bool(rev_compl_pair_file))
        self._ck(lib.pgrc_decode_set_order(self._h, C.byref(o)))

    def set_order_pair_streams(self, streams: dict, rev_compl_pair_file: bool = False) -> None:
        """the paired ORD order from the archive's pair-position streams (a dict as compressReadsPgPositions returns):
        the positions are decoded on the device into the context's order and never exist on the host"""
        s, keep = _pairpos_struct(streams)
        self._ck(lib.pgrc_decode_set_order_pair_streams(self._h, C.byref(s), int(bool(rev_compl_pair_file))))

    def set_order_positions(self, positions, rev_compl_pair_file: bool = False) -> None:
        """the single-file ORD order from orgIdx2PgPos as the archive holds it: an unsigned integer array whose dtype is the
        position width (uint32 or uint64; any other width is the library's to refuse), widened on the device"""
        a = np.ascontiguousarray(positions)
        assert a.dtype.kind == "u" and a.ndim == 1
        self._ck(lib.pgrc_decode_set_order_positions(self._h, _ptr(a), a.dtype.itemsize, a.size, int(bool(rev_compl_pair_file))))

    def decompressReadsPgPositions(self, streams: dict) -> np.ndarray:
        """SeparatedPseudoGenomePersistence::decompressReadsPgPositions (:582-673) on the device: the positions as
        n_total uint64, file-major ([p] the base read of pair p, [n_total/2 + p] its mate)"""
        s, keep = _pairpos_struct(streams)
        out = np.empty(int(s.n_total), dtype=np.uint64)
        self._ck(lib.pgrc_pairpos_decode(self._h, C.byref(s), _ptr(out)))
        return out

    def compressReadsPgPositions(self, org_idx_to_pos, pos_width: int) -> dict:
        """SeparatedPseudoGenomePersistence::compressReadsPgPositions (:445-574) on the device: org_idx_to_pos holds
        the mates interleaved ([2p] the base read of pair p, [2p+1] its mate); -> the eight streams by name (copies),
        n_total and pos_width"""
        op = np.ascontiguousarray(org_idx_to_pos, dtype=np.uint64)
        s = PairPosStreams()
        self._ck(lib.pgrc_pairpos_encode(self._h, _ptr(op), op.size, int(pos_width), C.byref(s)))
        try:
            out = _pairpos_dict(s)
        finally:
            lib.pgrc_pairpos_free(C.byref(s))
        return out

    def pairpos_timing(self) -> dict:
        t = PairPosTiming()
        t.struct_size = C.sizeof(PairPosTiming)
        self._ck(lib.pgrc_pairpos_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def compressReadsOrder(self, org_idx_parts, form: int) -> dict:
        """SeparatedPseudoGenomePersistence::compressReadsOrder (:220-339) on the device: org_idx_parts holds the orgIdx
        arrays of up to three reads lists (HQ, LQ, N; one array: a single list), which are never joined on the host;
        form is one of PGRC_PAIRORDER_*; -> the form's streams by name (copies; the streams the form does not write
        are absent), n_total and form"""
        if isinstance(org_idx_parts, np.ndarray):
            org_idx_parts = [org_idx_parts]
        parts = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in org_idx_parts]
        assert len(parts) <= 3
        ptrs, cnts = (_P * 3)(), (C.c_uint64 * 3)()
        for l, a in enumerate(parts):
            ptrs[l], cnts[l] = (a.ctypes.data if a.size else None), a.size
        s = PairOrderStreams()
        self._ck(lib.pgrc_pairorder_encode(self._h, ptrs, cnts, int(form), C.byref(s)))
        try:
            out = _pairorder_dict(s)
        finally:
            lib.pgrc_pairorder_free(C.byref(s))
        return out

    def pairorder_timing(self) -> dict:
        t = PairOrderTiming()
        t.struct_size = C.sizeof(PairOrderTiming)
        self._ck(lib.pgrc_pairorder_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def decompressReadsOrder(self, streams: dict) -> np.ndarray:
        """SeparatedPseudoGenomePersistence::decompressReadsOrder (:341-443) on the device: the streams of any form (a dict
        as compressReadsOrder returns) -> rlIdxOrder as n_total uint32"""
        s, keep = _pairorder_struct(streams)
        out = np.empty(int(s.n_total), dtype=np.uint32)
        self._ck(lib.pgrc_pairorder_decode(self._h, C.byref(s), _ptr(out)))
        return out

    def set_order_pair_order_streams(self, streams: dict, rev_compl_pair_file: bool = False) -> None:
        """the PE order from the archive's pair-order streams (a dict as compressReadsOrder returns): rlIdxOrder is decoded
        on the device into the context's order and never exists on the host"""
        s, keep = _pairorder_struct(streams)
        self._ck(lib.pgrc_decode_set_order_pair_order_streams(self._h, C.byref(s), int(bool(rev_compl_pair_file))))

    def pairorder_decode_timing(self) -> dict:
        t = PairOrderDecodeTiming()
        t.struct_size = C.sizeof(PairOrderDecodeTiming)
        self._ck(lib.pgrc_pairorder_get_decode_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def list_archive_encode(self, mis_cnt, mis_sym, mis_rev_off, fast_level: bool = False) -> dict:
        """SeparatedPseudoGenomeOutputBuilder::compressedBuild's reshaping of a list's mismatch streams (:905-952) on the
        device: counts, context codes and rev-coded offsets as pgrc_export_streams holds them -> zero_flags, nonzero_cnt,
        mis_sym (exclusive codes), bases_order, props and dests (a list: dests[c] the offsets of the entries with c
        mismatches, [0] empty), all copies"""
        x, keep = _export_struct(mis_cnt, mis_sym, mis_rev_off)
        s = ListArchiveStreams()
        self._ck(lib.pgrc_list_archive_encode(self._h, C.byref(x), int(bool(fast_level)), C.byref(s)))
        try:
            out = _list_archive_dict(s)
        finally:
            lib.pgrc_list_archive_free(C.byref(s))
        return out

    def add_list_archive(self, n_entries: int, streams: dict, text_base: int = 0, off=None, pos=None, rev_comp=None) -> None:
        """add_list with the list's mismatch streams in the archive's form (a dict as list_archive_encode returns): they go
        up as they are and the per-entry tables are rebuilt on the device"""
        a = DecodeList()
        a.struct_size = C.sizeof(DecodeList)
        a.text_base = int(text_base)
        a.n_entries = int(n_entries)
        keep = []
        if off is not None:
            off = np.ascontiguousarray(off)
            assert off.dtype in (np.uint8, np.uint16) and off.size == n_entries
            a.off, a.off_width = _ptr(off), off.dtype.itemsize
            keep.append(off)
        if pos is not None:
            pos = _arr(pos, np.uint64)
            a.pos = _ptr(pos)
            keep.append(pos)
        if rev_comp is not None:
            rev_comp = _arr(rev_comp, np.uint8)
            a.rev_comp = _ptr(rev_comp)
            keep.append(rev_comp)
        s, keep2 = _list_archive_struct(streams)
        self._ck(lib.pgrc_decode_add_list_archive(self._h, C.byref(a), C.byref(s)))

    def list_archive_timing(self) -> dict:
        t = ListArchiveTiming()
        t.struct_size = C.sizeof(ListArchiveTiming)
        self._ck(lib.pgrc_list_archive_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_ if k != "struct_size"}

    def row_count(self, file: int = 0) -> int:
        n = C.c_uint64(0)
        self._ck(lib.pgrc_decode_row_count(self._h, int(file), C.byref(n)))
        return n.value

    def rows(self, file: int = 0, first: int = 0, n: int | None = None, out=None) -> np.ndarray:
        """rows [first, first+n) of one output file of the current order, (n, L+1) uint8 (into `out` if given: any
        C-contiguous uint8 buffer of n*(L+1) bytes, e.g. a pinned torch tensor's numpy view)"""
        if n is None:
            n = self.row_count(file) - first
        L1 = self.readLength + 1
        if out is None:
            out = np.empty((n, L1), dtype=np.uint8)
        assert out.flags.c_contiguous and out.nbytes == n * L1
        self._ck(lib.pgrc_decode_rows(self._h, int(file), int(first), int(n), out.ctypes.data_as(_P)))
        return out.reshape(n, L1)

    def rows_device(self, file: int, first: int, n: int, dev_ptr: int) -> None:
        """rows into device memory (16-byte aligned), on the context's stream"""
        self._ck(lib.pgrc_decode_rows_device(self._h, int(file), int(first), int(n), _P(dev_ptr)))

    def timing(self) -> dict:
        t = DecodeTiming()
        self._ck(lib.pgrc_decode_get_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    # ---- the reference's writers (pgrc/pgrc-decoder.cpp)
    def writeAllReadsInSEMode(self) -> np.ndarray:
        """:137-239 -- every list in list order"""
        self.set_order(PGRC_DECODE_SE)
        return self.rows(0)

    def writeAllReadsInPEMode(self, rlIdxOrder, revComplPairFile: bool = False):
        """:241-383 -- file p holds rows i = p (mod 2) of rlIdxOrder; -> (file 1 rows, file 2 rows)"""
        ro = np.ascontiguousarray(rlIdxOrder, dtype=np.uint32)
        self.set_order(PGRC_DECODE_PE, ro.size, rl_idx_order=ro, rev_compl_pair_file=revComplPairFile)
        return self.rows(0), self.rows(1)

    def writeAllReadsInORDMode(self, orgIdx2PgPos, singleReadsMode: bool = True, revComplPairFile: bool = False):
        """:385-527 -- one row per original index; -> (rows,) or (file 1 rows, file 2 rows)"""
        op = np.ascontiguousarray(orgIdx2PgPos, dtype=np.uint64)
        self.set_order(PGRC_DECODE_ORD, op.size, org_idx_to_pos=op, paired=not singleReadsMode,
                       rev_compl_pair_file=revComplPairFile)
        return tuple(self.rows(p) for p in range(1 if singleReadsMode else 2))

    def verifier(self, kind: int = 0):
        """a pgrc_amd.Verifier of this job (text, lists and order set): IN_ORDER for an ORD job and MULTISET for SE and PE
        by default (include/pgrc_verify.h).  Close it before the job changes or the decoder closes."""
        from .verify import Verifier
        return Verifier(self, kind)

    def close(self) -> None:
        if self._h:
            lib.pgrc_decode_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compressReadsPgPositions(org_idx_to_pos, pos_width: int, device: int = -1) -> dict:
    """PgRCDecoder.compressReadsPgPositions on a context of its own"""
    dec = PgRCDecoder(1, device)
    try:
        return dec.compressReadsPgPositions(org_idx_to_pos, pos_width)
    finally:
        dec.close()


def decompressReadsPgPositions(streams: dict, device: int = -1) -> np.ndarray:
    """PgRCDecoder.decompressReadsPgPositions on a context of its own"""
    dec = PgRCDecoder(1, device)
    try:
        return dec.decompressReadsPgPositions(streams)
    finally:
        dec.close()


def compressReadsOrder(org_idx_parts, form: int, device: int = -1) -> dict:
    """PgRCDecoder.compressReadsOrder on a context of its own"""
    dec = PgRCDecoder(1, device)
    try:
        return dec.compressReadsOrder(org_idx_parts, form)
    finally:
        dec.close()


def decompressReadsOrder(streams: dict, ctx: PgRCDecoder | None = None, device: int = -1) -> np.ndarray:
    """PgRCDecoder.decompressReadsOrder on `ctx`, or on a context of its own"""
    if ctx is not None:
        return ctx.decompressReadsOrder(streams)
    dec = PgRCDecoder(1, device)
    try:
        return dec.decompressReadsOrder(streams)
    finally:
        dec.close()
