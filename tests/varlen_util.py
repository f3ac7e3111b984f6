"""Restatements of the reference's variable-length DNA coder (coders/VarLenDNACoder.cpp), the checkers of pgrc_amd/csrc/varlen.hip:

  parse_stream     what VarLenDNACoder::Compress writes: two header bytes, the book (writeBook), the payload
  Book             initUsing (:10-35): the codes and the look-up table over 27-bit keys, filled in index order
  encode_serial    encode (:55-104), the loop as it stands; a text shorter than 4 takes the tail rule from position 0
  encode_parallel  the same parse as tile maps {0..3} -> {0..3} folded in a tree (the form the device uses)
  decode           decode (:106-120)

plus the texts of the fixtures, re-derived from seeds (tests/golden/make_golden_varlen.py stores their digests and what the
reference made of them).  The books themselves are never written down here: they come out of the recorded streams."""
from __future__ import annotations

import glob
import hashlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LUT_MASK = 0x07FFFFFF
MAP_IDENTITY = (0, 1, 2, 3)
BOOK_IDS = (0, 1, 2)      # VarLenDNACoder::CODEBOOK_ID: AG_EXTENDED (the encoder's), SYNC_ON_A, AG_SHORT_EXTENDED

# (name, kind, seed, n): the generated texts of the fixtures
TEXT_CASES = [
    ("random", "random", 41, 30011),
    ("n_runs", "n_runs", 42, 9001),
    ("all_a", "all_a", 0, 40003),
    ("ac", "ac", 0, 5001),
    ("all_marks", "all_marks", 0, 500),       # (one code a symbol: the reference's output buffer holds 1412 + 0.53 n bytes for book and codes)
    ("alphabet", "alphabet", 0, 6004),
    ("n3", "random", 43, 3), ("n4", "random", 44, 4), ("n5", "random", 45, 5), ("n6", "random", 46, 6), ("n7", "random", 47, 7),
]


def make_text(kind: str, seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "random":                                    # ACGT with one '%' in 500
        t = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].copy()
        t[rng.random(n) < 1 / 500] = ord("%")
        return t
    if kind == "n_runs":
        t = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].copy()
        for at in rng.integers(0, max(n - 40, 1), size=max(n // 300, 1)):
            t[at:at + int(rng.integers(1, 40))] = ord("N")
        t[rng.random(n) < 1 / 400] = ord("%")
        return t
    unit = {"all_a": b"A", "ac": b"AC", "all_marks": b"%", "alphabet": b"ACGTN%"}[kind]
    return np.frombuffer((unit * (n // len(unit) + 1))[:n], np.uint8).copy()


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()[:16]


def joined_mapped(pgmap_npz) -> np.ndarray:
    """the joined mapped text HQ | LQ | N of a pgmap_* fixture: what matchPgsInPg hands to the coder"""
    return np.concatenate([np.asarray(pgmap_npz[f"mapped{p}"], dtype=np.uint8) for p in range(3)])


# ---------------------------------------------------------------------------------------------------- book and stream
class Book:
    def __init__(self, raw: bytes):
        """raw: the writeBook form, with or without the trailing NUL"""
        raw = bytes(raw)
        self.raw = raw.split(b"\0", 1)[0]
        self.codes = self.raw.split(b"\n")
        self.lut = {}
        for i, c in enumerate(self.codes):
            self.lut[int.from_bytes(c.ljust(4, b"\0")[:4], "little") & LUT_MASK] = i
        self.symbols = sorted(set(self.raw) - {ord("\n")})

    def look(self, key: int) -> int:
        return self.lut.get(key, 0)

    def check(self) -> None:
        """what pgrc_varlen_create demands"""
        assert len(self.codes) <= 256 and all(len(c) <= 4 for c in self.codes)
        assert len(self.codes[0]) == 1
        assert all(bytes([s]) in self.codes for s in self.symbols)
        assert len({s & 7 for s in self.symbols}) == len(self.symbols) and all(s & 7 for s in self.symbols)


def parse_stream(stream) -> tuple:
    """-> (mode, book id, Book, payload) of a whole Compress output"""
    b = bytes(np.asarray(stream, dtype=np.uint8).tobytes())
    end = b.index(b"\0", 2)
    return b[0], b[1], Book(b[2:end + 1]), b[end + 1:]


def load_fixtures() -> list:
    """-> [(name, text, {book id: whole stream})] of every varlen_*.npz; pgmap-derived texts come from the pgmap fixture"""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "varlen_*.npz"))):
        z = np.load(path)
        name = os.path.basename(path)[7:-4]
        src = z["source"].tobytes().decode()
        if src.startswith("pgmap_"):
            text = joined_mapped(np.load(os.path.join(GOLDEN, src + ".npz")))
        else:
            kind, seed, n = src.split(":")
            text = make_text(kind, int(seed), int(n))
        assert digest(text) == z["digest"].tobytes().decode(), f"{name}: text generator drifted"
        out.append((name, text, {int(k[5:]): z[k] for k in z.files if k.startswith("coded")}))
    return out


# ---------------------------------------------------------------------------------------------------- the coder
def encode_serial(book: Book, text) -> bytes:
    src = bytes(np.ascontiguousarray(text, dtype=np.uint8).tobytes())
    n, pos, out, look = len(src), 0, bytearray(), book.look
    while pos + 4 <= n:
        t = int.from_bytes(src[pos:pos + 4], "little") & LUT_MASK
        if look(t):
            out.append(look(t)); pos += 4
        elif look(t & 0xFFFFFF):
            out.append(look(t & 0xFFFFFF)); pos += 3
        elif look(t & 0xFFFF):
            out.append(look(t & 0xFFFF)); pos += 2
        else:
            out.append(look(t & 0xFF)); pos += 1
    while pos < n:
        t = int.from_bytes(src[pos:n].ljust(4, b"\0"), "little") & LUT_MASK & 0xFFFFFF
        if n - pos >= 3 and look(t):
            out.append(look(t)); pos += 3
        elif n - pos >= 2 and look(t & 0xFFFF):
            out.append(look(t & 0xFFFF)); pos += 2
        else:
            out.append(look(t & 0xFF)); pos += 1
    return bytes(out)


def steps_and_codes(book: Book, text):
    """step(pos) and the code emitted at pos, for every pos, as a function of text[pos, pos + 4) and n alone"""
    src = np.ascontiguousarray(text, dtype=np.uint8)
    n = src.size
    pad = np.concatenate([src, np.zeros(4, np.uint8)]).astype(np.uint32)
    t = pad[:n] | pad[1:n + 1] << 8 | pad[2:n + 2] << 16 | (pad[3:n + 3] & 7) << 24
    keys = np.array(sorted(book.lut), dtype=np.uint32)
    vals = np.array([book.lut[int(k)] for k in keys], dtype=np.uint8)

    def look(q):
        at = np.minimum(np.searchsorted(keys, q), keys.size - 1)
        return np.where(keys[at] == q, vals[at], 0).astype(np.uint8)

    rem = n - np.arange(n)
    f4 = np.where(rem >= 4, look(t), 0)
    f3 = np.where(rem >= 3, look(t & 0xFFFFFF), 0)
    f2 = np.where(rem >= 2, look(t & 0xFFFF), 0)
    f1 = look(t & 0xFF)
    step = np.where(f4 > 0, 4, np.where(f3 > 0, 3, np.where(f2 > 0, 2, 1)))
    code = np.where(f4 > 0, f4, np.where(f3 > 0, f3, np.where(f2 > 0, f2, f1)))
    return step.astype(np.int64), code.astype(np.uint8)


def compose(a, b):
    """the map "a, then b" """
    return tuple(b[a[e]] for e in range(4))


def exclusive_fold(maps):
    """out[i] = maps[0], then ..., then maps[i - 1] (the identity for i = 0), folded pairwise up a tree and handed down"""
    if len(maps) <= 1:
        return [MAP_IDENTITY] * len(maps)
    pairs = [compose(maps[i], maps[i + 1]) if i + 1 < len(maps) else maps[i] for i in range(0, len(maps), 2)]
    up = exclusive_fold(pairs)
    out = []
    for i in range(len(maps)):
        out.append(up[i // 2] if i % 2 == 0 else compose(up[i // 2], maps[i - 1]))
    return out


def tile_walk(step, n, lo, hi, entry):
    """the positions of the parse that enters tile [lo, hi) at lo + entry -> (positions inside the text, exit offset)"""
    pos, seen = lo + entry, []
    while pos < hi:
        if pos < n:
            seen.append(pos)
            pos += int(step[pos])
        else:
            pos += 1
    return seen, pos - hi


def encode_parallel(book: Book, text, tile: int = 64):
    """-> (payload, the fold of all tile maps applied to 0 = the parse's exit offset, tiles)"""
    step, code = steps_and_codes(book, text)
    n = step.size
    nt = (n + tile - 1) // tile
    maps = [tuple(tile_walk(step, n, t * tile, (t + 1) * tile, e)[1] for e in range(4)) for t in range(nt)]
    entries = [m[0] for m in exclusive_fold(maps)]
    out = []
    for t in range(nt):
        seen, _ = tile_walk(step, n, t * tile, (t + 1) * tile, entries[t])
        out.append(code[seen])
    total = MAP_IDENTITY
    for m in maps:
        total = compose(total, m)
    return (np.concatenate(out).tobytes() if out else b""), total[0], nt


def decode(book: Book, coded) -> bytes:
    codes = book.codes
    return b"".join(codes[c] if c < len(codes) else b"" for c in bytes(coded))


# ---------------------------------------------------------------------------------------------------- the source's constants
def source_constants() -> dict:
    """VL_* of varlen.hip and SCO_* of scanops.h, evaluated"""
    env = {}
    for fn in ("scanops.h", "varlen.hip"):
        src = open(os.path.join(ROOT, "pgrc_amd", "csrc", fn)).read()
        for name, expr in re.findall(r"^#define ((?:VL|SCO)_[A-Z0-9_]+) +([^/\n]+?) *(?://.*)?$", src, re.M):
            expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU][lL]*\b", r"\1", expr).replace("/", "//")
            try:
                env[name] = int(eval(expr, {}, dict(env)))
            except Exception:
                pass
    return env
