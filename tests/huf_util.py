"""The Huffman mode of the reference's coder type 5 (FSE_HUF_CODER; coders/FSECoder.cpp, coders/fse/huf_*.c) restated in
numpy / Python: the writer whose every choice is fixed here and which pgrc_amd/csrc/huf.hip follows byte for byte, and a reader
of everything the reference's writer may produce.  include/pgrc_huf.h describes the format; DESIGN.md 4.25 the rules.

The writer's rules (everything the format leaves open):
  the order     the present symbols by falling count, equal counts by rising symbol value: rank 0 is the most frequent
  the tree      two queues: the leaves from the last rank to the first, the inner nodes in the order they were made; the
                lighter head is taken, the leaf where both weigh the same; only the NUMBER of leaves of every depth is kept
  the limit     depths beyond table_log count as table_log; while the Kraft sum is too large, one code of length table_log is
                dropped and the longest shorter code is replaced by two codes one bit longer (one unit of the sum each time)
  the lengths   dealt out along the ranks, the shortest first
  the header    raw 4-bit weights when the highest present symbol is <= 128; else FSE-coded weights at table log 6 with the
                distribution fse_norm() gives; a header that does not fit in 127 bytes: the chunk is stored raw
  the verdict   one distinct symbol: RLE (1 byte); fewer than 12 bytes, or a coded chunk not shorter than the chunk: raw
"""
import numpy as np

MODE_HUF, MODE_FSE = 0, 1
ORDER_MAX, TABLE_LOG_MIN, TABLE_LOG_MAX, TABLE_LOG_READ_MAX = 17, 8, 11, 12
KIND_RAW, KIND_RLE, KIND_HUF = 0, 1, 2
FSE_HDR_LOG = 6


class HufError(ValueError):
    pass


def highbit(x: int) -> int:
    return int(x).bit_length() - 1


# ---------------------------------------------------------------------------------------------------- the writer: lengths
def code_lengths(count, table_log: int):
    """count[256] with at least two non-zero entries -> (lens[256], max_len)"""
    order = sorted((s for s in range(256) if count[s]), key=lambda s: (-int(count[s]), s))
    m = len(order)
    assert m >= 2 and table_log >= TABLE_LOG_MIN
    node_w, node_parent, leaf_parent = [], [], [0] * m
    leaf, head = m - 1, 0
    for k in range(m - 1):
        w = 0
        for _ in range(2):
            if leaf >= 0 and (head >= len(node_w) or int(count[order[leaf]]) <= node_w[head]):
                leaf_parent[leaf] = k
                w += int(count[order[leaf]])
                leaf -= 1
            else:
                node_parent[head] = k
                w += node_w[head]
                head += 1
        node_w.append(w)
        node_parent.append(-1)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    bl = [0] * (table_log + 1)
    for i in range(m):
        bl[min(depth[leaf_parent[i]] + 1, table_log)] += 1
    total = sum(bl[i] << (table_log - i) for i in range(1, table_log + 1))
    while total > (1 << table_log):
        bl[table_log] -= 1
        for i in range(table_log - 1, 0, -1):
            if bl[i]:
                bl[i] -= 1
                bl[i + 1] += 2
                break
        total -= 1
    lens = np.zeros(256, np.uint8)
    r = 0
    for ln in range(1, table_log + 1):
        for _ in range(bl[ln]):
            lens[order[r]] = ln
            r += 1
    return lens, max(i for i in range(1, table_log + 1) if bl[i])


def code_values(lens, max_len: int):
    """the values HUF_readDTableX1's fill order implies: the longest codes from 0 on, each shorter length from where the
    longer one ended, halved; within a length by rising symbol"""
    nb = np.bincount(lens, minlength=max_len + 2)
    start, low = [0] * (max_len + 2), 0
    for ln in range(max_len, 0, -1):
        start[ln] = low
        low = (low + int(nb[ln])) >> 1
    vals = np.zeros(256, np.uint32)
    for s in range(256):
        if lens[s]:
            vals[s] = start[lens[s]]
            start[lens[s]] += 1
    return vals


# ---------------------------------------------------------------------------------------------------- the writer: header
class BitsUp:
    """bits added from bit 0 of byte 0 upwards"""

    def __init__(self):
        self.v, self.n = 0, 0

    def add(self, value: int, nbits: int):
        self.v |= (int(value) & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def to_bytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fse_norm(cnt, total: int):
    """the shares of 64 table cells: max(1, cnt * 64 // total) for every weight that occurs; then, one cell at a time, the
    largest share (the lowest weight among equals) gains or loses a cell until the sum is 64.  One weight alone: it keeps 63
    and weight 0 (weight 1 if it is weight 0 itself) gets the last cell, because the format has no table of one symbol."""
    size = 1 << FSE_HDR_LOG
    norm = [max(1, c * size // total) if c else 0 for c in cnt]
    if sum(1 for c in cnt if c) == 1:
        norm[0 if not cnt[0] else 1] = 1
    s = sum(norm)
    while s != size:
        k = max(range(len(norm)), key=lambda i: (norm[i], -i))
        d = 1 if s < size else -1
        norm[k] += d
        s += d
    return norm


def fse_spread(norm, tl: int):
    """FSE_buildDTable's layout (fse_decompress.c:85-123) -> (symbol, nbBits, newState) per cell"""
    size = 1 << tl
    sym, high = [0] * size, size - 1
    nxt = []
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
        nxt.append(1 if c == -1 else c)
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    if pos:
        raise HufError("weight header: the FSE table's counts do not fill the table")
    nb, base = [0] * size, [0] * size
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb[u] = tl - highbit(x)
        base[u] = (x << nb[u]) - size
    return sym, nb, base


def fse_weights(weights) -> bytes:
    """the FSE form of a weight header without its size byte: the NCount table (FSE_readNCount, entropy_common.c:40-144) and
    the two-state stream FSE_decompress_usingDTable reads (fse_decompress.c:178-238)"""
    nw = len(weights)
    cnt = [0] * 12
    for w in weights:
        cnt[w] += 1
    norm = fse_norm(cnt, nw)
    last = max(i for i in range(12) if norm[i])
    b = BitsUp()
    b.add(FSE_HDR_LOG - 5, 4)
    remaining, threshold, nbits, s, prev0 = (1 << FSE_HDR_LOG) + 1, 1 << FSE_HDR_LOG, FSE_HDR_LOG + 1, 0, False
    while remaining > 1:
        assert s <= last
        if prev0:
            run = 0
            while norm[s + run] == 0:
                run += 1
            s += run
            while run >= 24:
                b.add(0xFFFF, 16)
                run -= 24
            while run >= 3:
                b.add(3, 2)
                run -= 3
            b.add(run, 2)
        c = norm[s]
        s += 1
        v, mx = c + 1, 2 * threshold - 1 - remaining
        if v < mx:
            b.add(v, nbits - 1)
        elif v < threshold:
            b.add(v, nbits)
        else:
            b.add(v + mx, nbits)
        remaining -= c
        prev0 = c == 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    head = b.to_bytes()
    # the stream: symbol i belongs to state i & 1; the last symbol of each state starts in the first cell that shows it, and
    # every earlier one in the cell whose interval holds the state that follows
    sym, nb, base = fse_spread(norm, FSE_HDR_LOG)
    cells = [[u for u in range(1 << FSE_HDR_LOG) if sym[u] == w] for w in range(12)]
    st = [None, None]
    out = BitsUp()
    for i in range(nw - 1, -1, -1):
        w, cur = weights[i], st[i & 1]
        if cur is None:
            st[i & 1] = cells[w][0]
            continue
        u = next(u for u in cells[w] if base[u] <= cur < base[u] + (1 << nb[u]))
        out.add(cur - base[u], nb[u])
        st[i & 1] = u
    out.add(st[1], FSE_HDR_LOG)
    out.add(st[0], FSE_HDR_LOG)
    out.add(1, 1)
    return head + out.to_bytes()


def weight_header(lens, max_len: int, max_sym: int):
    """HUF_writeCTable's two forms (huf_compress.c:114-147), or None where the FSE form does not fit in 127 bytes"""
    w = [int(max_len + 1 - lens[s]) if lens[s] else 0 for s in range(max_sym)]
    if max_sym <= 128:
        w2 = w + [0]
        return bytes([127 + max_sym]) + bytes((w2[i] << 4) | w2[i + 1] for i in range(0, max_sym, 2))
    body = fse_weights(w)
    return bytes([len(body)]) + body if len(body) <= 127 else None


# ---------------------------------------------------------------------------------------------------- the writer: streams
def encode_stream(seg, lens, vals) -> bytes:
    """one segment, its first symbol highest: symbol i at the bit offset that is the sum of the lengths behind it, the end
    mark above everything (HUF_compress1X_usingCTable_internal_body, huf_compress.c:457-512; BIT_closeCStream)"""
    ln = lens[seg].astype(np.int64)
    total = int(ln.sum())
    off = total - np.cumsum(ln)
    words = np.zeros((total + 1 + 63) // 32 + 2, np.uint64)
    v = vals[seg].astype(np.uint64) << (off & 31).astype(np.uint64)
    np.add.at(words, off >> 5, v & np.uint64(0xFFFFFFFF))
    np.add.at(words, (off >> 5) + 1, v >> np.uint64(32))
    words[total >> 5] += np.uint64(1 << (total & 31))
    return words.astype("<u4").tobytes()[:(total + 8) // 8]


def chunk_plan(chunk, table_log: int):
    """-> (kind, header bytes, lens, vals, segment byte sizes, coded size) of one chunk"""
    n = chunk.size
    count = np.bincount(chunk, minlength=256)
    if int(count.max()) == n:
        return KIND_RLE, b"", None, None, None, 1
    if n < 12:
        return KIND_RAW, b"", None, None, None, n
    lens, max_len = code_lengths(count, table_log)
    hdr = weight_header(lens, max_len, int(np.flatnonzero(count)[-1]))
    if hdr is None:
        return KIND_RAW, b"", None, None, None, n
    seg = (n + 3) // 4
    sizes = [(int(lens[chunk[k * seg:min((k + 1) * seg, n)]].astype(np.int64).sum()) + 8) // 8 for k in range(4)]
    csize = len(hdr) + 6 + sum(sizes)
    if csize >= n:
        return KIND_RAW, b"", None, None, None, n
    return KIND_HUF, hdr, lens, code_values(lens, max_len), sizes, csize


def encode_chunk(chunk, table_log: int) -> bytes:
    kind, hdr, lens, vals, sizes, csize = chunk_plan(chunk, table_log)
    if kind == KIND_RLE:
        return chunk[:1].tobytes()
    if kind == KIND_RAW:
        return chunk.tobytes()
    n, seg = chunk.size, (chunk.size + 3) // 4
    streams = [encode_stream(chunk[k * seg:min((k + 1) * seg, n)], lens, vals) for k in range(4)]
    assert [len(s) for s in streams] == sizes
    out = hdr + b"".join(int(s).to_bytes(2, "little") for s in sizes[:3]) + b"".join(streams)
    assert len(out) == csize
    return out


def as_u8(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)


def frame(chunks, block_order: int, table_log: int, mode: int = MODE_HUF) -> bytes:
    """FSECompress's frame (FSECoder.cpp:34-78) around coded chunks: every chunk but the last with its size in front"""
    out = [bytes([mode, block_order, 255, table_log])]
    for k, c in enumerate(chunks):
        if k + 1 < len(chunks):
            out.append(len(c).to_bytes(4, "little"))
        out.append(bytes(c))
    return b"".join(out)


def split(data, block_order: int):
    a = as_u8(data)
    return [a[i:i + (1 << block_order)] for i in range(0, a.size, 1 << block_order)]


def encode(data, block_order: int = ORDER_MAX, table_log: int = TABLE_LOG_MAX) -> bytes:
    if not 1 <= block_order <= ORDER_MAX or not TABLE_LOG_MIN <= table_log <= TABLE_LOG_MAX:
        raise HufError("block_order 1 .. 17, table_log 8 .. 11")
    return frame([encode_chunk(c, table_log) for c in split(data, block_order)], block_order, table_log)


def bound(n: int, block_order: int) -> int:
    return 4 + n + 4 * max(((n + (1 << block_order) - 1) >> block_order) - 1, 0)


# ---------------------------------------------------------------------------------------------------- the reader
class BitsDown:
    """a stream read from its end mark downwards (BIT_initDStream / BIT_readBits, bitstream.h); bits below bit 0 are zero"""

    def __init__(self, buf: bytes, what: str):
        if not buf or not buf[-1]:
            raise HufError(f"{what}: no end mark")
        self.v = int.from_bytes(buf, "little")
        self.left = 8 * (len(buf) - 1) + highbit(buf[-1])

    def peek(self, nbits: int) -> int:
        if self.left >= nbits:
            return (self.v >> (self.left - nbits)) & ((1 << nbits) - 1)
        return ((self.v & ((1 << max(self.left, 0)) - 1)) << (nbits - max(self.left, 0))) & ((1 << nbits) - 1)

    def skip(self, nbits: int):
        self.left -= nbits


def read_ncount(buf: bytes):
    """FSE_readNCount (entropy_common.c:40-144) as a plain bit stream -> (table log, counts of the 12 weights, bytes read)"""
    v, pos = int.from_bytes(buf, "little"), 0

    def peek(nbits):
        return (v >> pos) & ((1 << nbits) - 1)
    tl = peek(4) + 5
    pos += 4
    if tl > FSE_HDR_LOG:
        raise HufError("weight header: FSE table log above 6")
    remaining, threshold, nbits, s, prev0 = (1 << tl) + 1, 1 << tl, tl + 1, 0, False
    norm = [0] * 12
    while remaining > 1 and s <= 255:
        if prev0:
            while peek(16) == 0xFFFF:
                s += 24
                pos += 16
            while peek(2) == 3:
                s += 3
                pos += 2
            s += peek(2)
            pos += 2
            if s > 255:
                raise HufError("weight header: zero run past the last symbol")
        mx = 2 * threshold - 1 - remaining
        if peek(nbits - 1) < mx:
            c = peek(nbits - 1)
            pos += nbits - 1
        else:
            c = peek(nbits)
            if c >= threshold:
                c -= mx
            pos += nbits
        c -= 1
        remaining -= abs(c)
        if c and s >= 12:
            raise HufError("weight header: a share for a weight above 11")
        if s < 12:
            norm[s] = c
        s += 1
        prev0 = c == 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        if pos > 8 * len(buf):
            raise HufError("weight header: the FSE table runs past the header")
    if remaining != 1:
        raise HufError("weight header: the FSE table's counts do not add up")
    return tl, norm, (pos + 7) // 8


def read_fse_weights(buf: bytes):
    tl, norm, used = read_ncount(buf)
    sym, nb, base = fse_spread(norm, tl)
    if used >= len(buf):
        raise HufError("weight header: no FSE stream")
    b = BitsDown(buf[used:], "weight header")
    if b.left < 2 * tl:
        raise HufError("weight header: the FSE stream is shorter than its two states")
    st = []
    for _ in range(2):
        st.append(b.peek(tl))
        b.skip(tl)
    out, i = [], 0
    while True:
        if len(out) > 253:
            raise HufError("weight header: more than 255 weights")
        u = st[i & 1]
        out.append(sym[u])
        if nb[u] > b.left:
            out.append(sym[st[(i + 1) & 1]])
            return out
        st[i & 1] = base[u] + b.peek(nb[u])
        b.skip(nb[u])
        i += 1


def read_stats(chunk: bytes):
    """HUF_readStats (entropy_common.c:154-215) -> (weights with the implied last one, table log, header bytes)"""
    h = chunk[0]
    if h >= 128:
        nw, used = h - 127, 1 + (h - 127 + 1) // 2
        if used > len(chunk):
            raise HufError("weight header: cut short")
        w = []
        for x in chunk[1:used]:
            w += [x >> 4, x & 15]
        w = w[:nw]
    else:
        used = 1 + h
        if used > len(chunk):
            raise HufError("weight header: cut short")
        w = read_fse_weights(chunk[1:used])
    if any(x >= 12 for x in w):
        raise HufError("weight header: a weight above 11")
    total = sum((1 << x) >> 1 for x in w)
    if not total:
        raise HufError("weight header: no weight")
    tl = highbit(total) + 1
    if tl > TABLE_LOG_READ_MAX:
        raise HufError("weight header: table log above 12")
    rest = (1 << tl) - total
    if rest & (rest - 1):
        raise HufError("weight header: the weights' sum leaves no power of two for the last symbol")
    w = w + [highbit(rest) + 1]
    ones = sum(1 for x in w if x == 1)
    if ones < 2 or ones & 1:
        raise HufError("weight header: an odd number of longest codes")
    return w, tl, used


def decode_table(w, tl: int):
    """HUF_readDTableX1_wksp's table (huf_decompress.c:151-183): by rising weight, within a weight by rising symbol"""
    sym, nb = np.zeros(1 << tl, np.uint8), np.zeros(1 << tl, np.uint8)
    at = 0
    for weight in range(1, tl + 1):
        for s, x in enumerate(w):
            if x == weight:
                span = 1 << (weight - 1)
                sym[at:at + span] = s
                nb[at:at + span] = tl + 1 - weight
                at += span
    assert at == 1 << tl
    return sym.tolist(), nb.tolist()


def decode_chunk(chunk: bytes, n: int) -> bytes:
    """HUF_decompress (huf_decompress.c:1056-1080) and the four-stream body (:262-354)"""
    c = len(chunk)
    if c == 0 or c > n:
        raise HufError(f"a coded chunk of {c} bytes for {n}")
    if c == n:
        return bytes(chunk)
    if c == 1:
        return bytes(chunk) * n
    w, tl, used = read_stats(chunk)
    body = chunk[used:]
    seg = (n + 3) // 4
    if len(body) < 10 or 3 * seg > n:
        raise HufError("a Huffman chunk without room for its jump table and four streams")
    sizes = [int.from_bytes(body[2 * k:2 * k + 2], "little") for k in range(3)]
    if 6 + sum(sizes) >= len(body):
        raise HufError("jump table: the segments' sizes exceed the chunk")
    sizes.append(len(body) - 6 - sum(sizes))
    sym, nb = decode_table(w, tl)
    out, at = [], 6
    for k in range(4):
        count = seg if k < 3 else n - 3 * seg
        b = BitsDown(body[at:at + sizes[k]], f"stream {k}")
        at += sizes[k]
        o = bytearray(count)
        for i in range(count):
            u = b.peek(tl)
            o[i] = sym[u]
            b.skip(nb[u])
        if b.left:
            raise HufError(f"stream {k}: ends {'early' if b.left < 0 else 'late'}")
        out.append(bytes(o))
    return b"".join(out)


def walk(payload: bytes, n: int):
    """FSEUncompress's walk over the frame (FSECoder.cpp:82-135) -> (block_order, [(offset, coded size, chunk length)])"""
    if len(payload) < 4:
        raise HufError("frame: shorter than its four props bytes")
    mode, order = payload[0], payload[1]
    if mode != MODE_HUF:
        raise HufError(f"frame: mode {mode} is not the Huffman mode")
    if order > ORDER_MAX:
        raise HufError(f"frame: block order {order} above 17")
    out, at, left = [], 4, n
    while left:
        clen = min(left, 1 << order)
        if clen < left:
            if at + 4 > len(payload):
                raise HufError("frame: cut inside a chunk's size")
            size = int.from_bytes(payload[at:at + 4], "little")
            at += 4
        else:
            size = len(payload) - at
        if size < 1 or size > clen or at + size > len(payload):
            raise HufError(f"frame: chunk {len(out)} has a coded size of {size} for {clen} bytes, {len(payload) - at} left")
        out.append((at, size, clen))
        at += size
        left -= clen
    if at != len(payload):
        raise HufError("frame: bytes behind the last chunk")
    return order, out


def decode(payload, n: int) -> bytes:
    payload = bytes(payload)
    return b"".join(decode_chunk(payload[at:at + size], clen) for at, size, clen in walk(payload, n)[1])


# ---------------------------------------------------------------------------------------------------- the tests' sources
def fib_counts(nsym: int = 256, cap: int = 1 << 17):
    """counts whose free Huffman tree is deeper than 11: Fibonacci numbers while they fit, ones for the rest"""
    c, a, b = [], 1, 1
    while a + sum(c) < cap // 2 and len(c) < 24:
        c.append(a)
        a, b = b, a + b
    return (c + [1] * nsym)[:nsym]


def source(kind: str, n: int, seed: int = 1) -> np.ndarray:
    """the alphabets of the tests, n bytes each"""
    rng = np.random.default_rng(seed)
    if kind == "one":
        return np.full(n, 0x41, np.uint8)
    if kind == "two":
        return np.where(rng.random(n) < 0.999, 3, 200).astype(np.uint8)
    if kind == "four":
        return np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, size=n, p=[0.5, 0.25, 0.15, 0.1])]
    if kind in ("s129", "s130"):
        m = 129 if kind == "s129" else 130
        p = 0.97 ** np.arange(m)
        a = rng.choice(m, size=n, p=p / p.sum()).astype(np.uint8)
        a[:m] = np.arange(m)[:n]                             # every symbol of the alphabet, where the length allows it
        return a
    if kind == "geo":
        p = 0.96 ** np.arange(256)
        a = rng.choice(256, size=n, p=p / p.sum()).astype(np.uint8)
        a[:256] = rng.permutation(256)[:n]
        return a
    if kind == "fib":
        c = np.array(fib_counts(256, max(n, 512)), np.float64)
        a = np.repeat(np.arange(256), np.maximum((c * n / c.sum()).astype(np.int64), 1))[:n]
        a = np.concatenate([a, np.zeros(n - a.size, np.int64)]).astype(np.uint8)
        return rng.permutation(a)
    if kind == "uniform":
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    raise KeyError(kind)


KINDS = ("one", "two", "four", "s129", "s130", "geo", "fib", "uniform")


def mixed(n: int, block_order: int, seed: int = 5) -> np.ndarray:
    """chunks that take the alphabets in turn: a table per chunk"""
    step = 1 << block_order
    return np.concatenate([source(KINDS[(i // step) % len(KINDS)], min(step, n - i), seed + i // step) for i in range(0, n, step)])


def load_golden():
    """tests/golden/huf_streams.npz (make_golden_huf.py) -> [(name, block_order, table_log, source, the reference's frame)]"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "huf_streams.npz"))
    out = []
    for key in sorted(k for k in z.files if k.endswith("/src")):
        _, kind, order, tl, _ = key.split("/")
        out.append((key[:-4], int(order), int(tl), z[key], z[key[:-3] + "frame"].tobytes()))
    return out


# the shapes of the CPU tests against the reference: (block_order, lengths)
REF_SHAPES = ((10, (1, 2, 11, 12, 13, 1023, 1024, 1025, 2048, 2057, 2058, 2059, 2060, 2061, 2062, 2063, 3000)), (12, (5000, 12289)),
              (17, (70001, 131072, 140000)))

_REF = None


def ref_lib():
    """HUF_compress2 and HUF_decompress of the compiled reference (oracle/_ref), or None"""
    global _REF
    import ctypes as C
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libpgrc_ref.so")
    if _REF is None and os.path.exists(path):
        _REF = C.CDLL(path)
        _REF.HUF_compress2.restype = _REF.HUF_decompress.restype = C.c_size_t
        _REF.HUF_compress2.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint]
        _REF.HUF_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    return _REF


def ref_compress_chunk(chunk, table_log: int = 11):
    """HUF_compress2 on one chunk -> its bytes (one byte for RLE), or None where it refuses (returns 0)"""
    import ctypes as C
    a = np.ascontiguousarray(chunk, np.uint8)
    cap = a.size + 1024
    dst = C.create_string_buffer(cap)
    r = ref_lib().HUF_compress2(dst, cap, a.ctypes.data, a.size, 255, table_log)
    assert r < (1 << 62), "HUF_compress2 reports an error"
    if r == 0:
        return None
    return a[:1].tobytes() if r == 1 else dst.raw[:r]


def ref_decompress_chunk(coded: bytes, n: int):
    import ctypes as C
    dst = C.create_string_buffer(max(n, 1))
    r = ref_lib().HUF_decompress(dst, n, coded, len(coded))
    return dst.raw[:n] if r == n else None
