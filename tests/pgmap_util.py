"""numpy restatements of the reference's Pg-vs-Pg marking and its inverse (matching/SimplePgMatcher.cpp), the checkers
of pgrc_decode_set_mapped_text:

  mark_and_remove      markAndRemoveExactMatches (:65-144) with correctDestPositionDueToRevComplMatching (:58-61) and
                       resolveMappingCollisionsInTheSameText (:157-171): the mapped text, the offsets stream (4 or 8
                       bytes per mark) and the byte-frugal lengths stream
  restore_matched_pg   restoreMatchedPg (:308-343), kept literal (a growing bytearray, find('%'), substr, reverse
                       complement), so that it gives the expected output for any bytes
  restore_matched_pgs  restoreMatchedPgs (:259-306) over the three parts

plus the byte-frugal coder (utils/helper.h:209-219, helper.cpp:179-187), complementsLut (helper.cpp:247-276) and
builders of hand-made mapped texts and streams."""
from __future__ import annotations

import numpy as np

MATCH_MARK = ord("%")
UINT32_MAX = 0xFFFFFFFF


def _complements_lut() -> bytes:
    lut = bytearray(256)
    for a, b in (("A", "T"), ("C", "G"), ("G", "C"), ("T", "A"), ("N", "N"), ("U", "A"), ("Y", "R"), ("R", "Y"),
                 ("K", "M"), ("M", "K"), ("B", "V"), ("D", "H"), ("H", "D"), ("V", "B")):
        lut[ord(a)] = ord(b)
        lut[ord(a.lower())] = ord(b)
    return bytes(lut)


COMPLEMENTS = _complements_lut()
COMPLEMENTS_NP = np.frombuffer(COMPLEMENTS, dtype=np.uint8)


def reverse_complement(b: bytes) -> bytes:
    return bytes(b).translate(COMPLEMENTS)[::-1]


def revcomp_np(a: np.ndarray) -> np.ndarray:
    return COMPLEMENTS_NP[np.ascontiguousarray(a, dtype=np.uint8)[::-1]]


# ---------------------------------------------------------------------------------------------------- byte-frugal
def write_uint_byte_frugal(out: bytearray, value: int) -> None:
    value &= (1 << 64) - 1
    while value >= 128:
        out.append(128 + value % 128)
        value //= 128
    out.append(value)


def read_uint_byte_frugal(buf: bytes, at: int, bits: int = 64):
    """-> (value, next position); the value modulo 2^bits as the reference's t_val accumulates it"""
    value, base = 0, 1
    while True:
        if at >= len(buf):
            raise ValueError("a byte-frugal value runs past its stream's end")
        y = buf[at]
        at += 1
        value += base * (y % 128)
        base *= 128
        if y < 128:
            return value % (1 << bits), at


def frugal_stream(values) -> bytes:
    out = bytearray()
    for v in values:
        write_uint_byte_frugal(out, int(v))
    return bytes(out)


# ---------------------------------------------------------------------------------------------------- the encoder side
def mark_and_remove(dest, matches, dest_is_src: bool, rev_compl: bool, min_len: int, src_len: int):
    """markAndRemoveExactMatches.  dest: the pseudogenome being mapped (uint8); matches: (n, 3) (posSrcText, length,
    posDestText) as matchTexts reported them for SimplePgMatcher's query text (the reverse complement of dest when
    rev_compl); src_len: the HQ length (the offset width).  -> (mapped, map_off, map_len) as bytes."""
    dest = np.ascontiguousarray(dest, dtype=np.uint8)
    G = dest.size
    m = np.asarray(matches, dtype=np.uint64).reshape(-1, 3)
    src, ln, dst = (m[:, 0].astype(np.int64), m[:, 1].astype(np.int64), m[:, 2].astype(np.int64))
    if rev_compl:                                            # correctDestPositionDueToRevComplMatching
        dst = G - (dst + ln)
    if dest_is_src:                                          # resolveMappingCollisionsInTheSameText
        swap = src > dst
        src, dst = np.where(swap, dst, src), np.where(swap, src, dst)
        if rev_compl:
            over = src + ln > dst
            margin = np.where(over, (src + ln - dst + 1) // 2, 0)
            ln = ln - margin
            dst = dst + margin
    order = np.lexsort((ln, src, dst))                       # sort by (posDestText, posSrcText, length) ...
    trip = np.stack([dst[order], src[order], ln[order]], axis=1)
    if trip.shape[0]:
        keep = np.ones(trip.shape[0], dtype=bool)            # ... and unique
        keep[1:] = np.any(trip[1:] != trip[:-1], axis=1)
        trip = trip[keep]
    pos = 0
    marks = []                                               # (posDest, posSrc, length) of the kept matches
    for d, s, L in trip.tolist():
        if d < pos:
            overflow = pos - d
            if overflow >= L:
                continue
            L -= overflow
            d += overflow
            if not rev_compl:
                s += overflow
        if L < min_len:
            continue
        marks.append((d, s, L))
        pos = d + L
    width = 4 if src_len <= UINT32_MAX else 8
    off = bytearray()
    lens = bytearray()
    write_uint_byte_frugal(lens, min_len)
    for d, s, L in marks:
        off += int(s).to_bytes(width, "little")
        write_uint_byte_frugal(lens, L - min_len)
    covered = np.zeros(G + 1, dtype=np.int64)
    if marks:
        mk = np.asarray(marks, dtype=np.int64)
        np.add.at(covered, mk[:, 0], 1)
        np.add.at(covered, mk[:, 0] + mk[:, 2], -1)
        cov = np.cumsum(covered)[:G] > 0
        kept = dest[~cov]
        at = mk[:, 0] - np.concatenate([[0], np.cumsum(mk[:, 2])[:-1]])
        mapped = np.insert(kept, at, MATCH_MARK)
    else:
        mapped = dest.copy()
    return mapped.tobytes(), bytes(off), bytes(lens)


def no_matcher_streams():
    """what markAndRemoveExactMatches writes when the HQ is shorter than the target length (no matcher): no streams"""
    return b"", b""


# ---------------------------------------------------------------------------------------------------- the decoder side
def restore_matched_pg(src: bytearray | bytes, org_src_len: int, dest: bytes, map_off: bytes, map_len: bytes,
                       rev_compl: bool = True, src_is_dest: bool = False) -> bytes:
    """restoreMatchedPg, literally: with src_is_dest the marks copy from the text being built"""
    std = org_src_len <= UINT32_MAX
    width = 4 if std else 8
    res = bytearray()
    srcbuf = res if src_is_dest else bytes(src)
    dest = bytes(dest)
    pos_dest = 0
    if len(map_len):
        min_len, lat = read_uint_byte_frugal(map_len, 0, 32)
    else:
        min_len, lat = 0, 0                  # an empty stream: read() fails, yByte stays 0
    oat = 0
    while True:
        mark = dest.find(b"%", pos_dest)
        if mark < 0:
            break
        res += dest[pos_dest:mark]
        pos_dest = mark + 1
        if oat + width > len(map_off):
            raise ValueError("offsets stream too short")
        sp = int.from_bytes(map_off[oat:oat + width], "little")
        oat += width
        v, lat = read_uint_byte_frugal(map_len, lat, 64)
        L = (v + min_len) % (1 << 64)
        if sp > len(srcbuf):
            raise ValueError("substr past the source end")
        piece = bytes(srcbuf[sp:sp + L])        # std::string::substr clips at the end
        res += reverse_complement(piece) if rev_compl else piece
    res += dest[pos_dest:]
    return bytes(res)


def restore_matched_pgs(mapped: bytes, mapped_lens, org_hq_len: int, map_off, map_len, rev_compl: bool = True):
    """restoreMatchedPgs -> (hq, lq, n) restored"""
    h, l, _ = (int(x) for x in mapped_lens)
    mapped = bytes(mapped)
    parts = (mapped[:h], mapped[h:h + l], mapped[h + l:])
    hq = restore_matched_pg(b"", org_hq_len, parts[0], map_off[0], map_len[0], rev_compl, True)
    lq = restore_matched_pg(hq, org_hq_len, parts[1], map_off[1], map_len[1], rev_compl)
    nn = restore_matched_pg(hq, org_hq_len, parts[2], map_off[2], map_len[2], rev_compl) if parts[2] else b""
    return hq, lq, nn


def hq_sources_valid(mapped_hq: bytes, map_off: bytes, map_len: bytes, org_hq_len: int) -> bool:
    """every HQ mark's source ends at or before the mark's output position (the device rejects the rest; the reference
    would clip a forward self-overlap)"""
    width = 4 if org_hq_len <= UINT32_MAX else 8
    marks = [i for i, c in enumerate(mapped_hq) if c == MATCH_MARK]
    if not marks:
        return True
    min_len, at = read_uint_byte_frugal(map_len, 0, 32)
    out_before = 0                               # lengths of the earlier matches
    for k, mp in enumerate(marks):
        off = int.from_bytes(map_off[k * width:(k + 1) * width], "little")
        v, at = read_uint_byte_frugal(map_len, at, 64)
        L = v + min_len
        opos = mp - k + out_before
        if off + L > opos:
            return False
        out_before += L
    return True


# ---------------------------------------------------------------------------------------------------- hand-made input
def build_part(pieces, min_len: int = 0, width: int = 4):
    """pieces: bytes (literals) and (offset, length) marks, in output order -> (mapped, map_off, map_len)"""
    mapped = bytearray()
    off = bytearray()
    lens = bytearray()
    marks = [p for p in pieces if not isinstance(p, (bytes, bytearray))]
    if marks:
        write_uint_byte_frugal(lens, min_len)
    for p in pieces:
        if isinstance(p, (bytes, bytearray)):
            mapped += p
        else:
            o, L = p
            mapped.append(MATCH_MARK)
            off += int(o).to_bytes(width, "little")
            write_uint_byte_frugal(lens, L - min_len)
    return bytes(mapped), bytes(off), bytes(lens)


def join_parts(parts):
    """[(mapped, off, len)] x 3 -> (joined mapped, mapped_lens, offs, lens)"""
    return (b"".join(p[0] for p in parts), [len(p[0]) for p in parts], [p[1] for p in parts], [p[2] for p in parts])


# ---------------------------------------------------------------------------------------------------- synthetic texts
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_texts(seed: int, G: int, G_lq: int, G_n: int, nrep: int = 40, chains: int = 0, chain_depth: int = 4,
               low_complexity: bool = False):
    """(hq, lq, n) uint8 texts: a random HQ with planted copies on both strands (and, with `chains`, reverse-complement
    copies of reverse-complement copies, chain_depth deep), an LQ and an N text that carry copies of HQ stretches (the N
    text also runs of N)"""
    rng = np.random.default_rng(seed)
    hq = rng.choice(ACGT, size=G)
    if low_complexity and G > 12000:
        hq[2000:6000] = ord("A")
        hq[8000:11000] = np.resize(np.frombuffer(b"ACG", dtype=np.uint8), 3000)
    for _ in range(nrep if G > 1000 else 0):
        L = int(rng.integers(60, 800))
        s, d = int(rng.integers(0, G - L)), int(rng.integers(0, G - L))
        seg = hq[s:s + L].copy()
        hq[d:d + L] = revcomp_np(seg) if rng.random() < 0.6 else seg
    for _ in range(chains):
        L = int(rng.integers(300, 1500))
        at = int(rng.integers(0, G // 4))
        seg = hq[at:at + L].copy()
        step = (G - at - L) // (chain_depth + 1)
        for k in range(chain_depth):
            at += int(rng.integers(L, max(L + 1, step)))
            if at + L > G:
                break
            seg = revcomp_np(seg)
            hq[at:at + L] = seg

    def other(size, n_runs):
        t = rng.choice(ACGT, size=size)
        if low_complexity and size > 4000:
            t[500:1800] = ord("T")
            t[2000:3200] = np.resize(np.frombuffer(b"CGT", dtype=np.uint8), 1200)
        for _ in range(size // 600 if G > 1000 else 0):
            L = min(int(rng.integers(50, 700)), G - 1, size - 1)
            s, d = int(rng.integers(0, G - L)), int(rng.integers(0, size - L))
            seg = hq[s:s + L].copy()
            t[d:d + L] = revcomp_np(seg) if rng.random() < 0.7 else seg
        for _ in range(n_runs):
            p = int(rng.integers(0, size - 4))
            t[p:p + int(rng.integers(1, 5))] = ord("N")
        return t

    lq = other(G_lq, 0) if G_lq else np.zeros(0, np.uint8)
    nn = other(G_n, G_n // 200) if G_n else np.zeros(0, np.uint8)
    return hq, lq, nn


def map_all(hq, lq, nn, match_fn, target_len: int, rev_compl: bool = True):
    """the three parts mapped as SimplePgMatcher::matchPgsInPg maps them (LQ, N, then HQ against itself), the matches
    from match_fn(src, query_text, dest_is_src, rev_compl) -> (n, 3).  -> (mapped, mapped_lens, offs, lens, matches)"""
    hq, lq, nn = (np.ascontiguousarray(x, dtype=np.uint8) for x in (hq, lq, nn))
    parts, found = [], []
    for dest, dis in ((hq, True), (lq, False), (nn, False)):
        m = np.zeros((0, 3), np.uint64)
        if hq.size < target_len or (dest is nn and dest.size == 0):
            # no matcher: empty streams; an empty N part: its streams are not stored (restoreMatchedPgs, :286-289)
            parts.append((dest.tobytes(), b"", b""))
        else:
            if dest.size:
                q = revcomp_np(dest) if rev_compl else dest
                m = np.asarray(match_fn(hq, q, dis, rev_compl), dtype=np.uint64).reshape(-1, 3)
            parts.append(mark_and_remove(dest, m, dis, rev_compl, target_len, hq.size))
        found.append(m)
    mapped, lens_m, offs, lns = join_parts(parts)
    return mapped, lens_m, offs, lns, found
