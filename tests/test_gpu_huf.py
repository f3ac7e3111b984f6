"""pgrc_amd.HufCoder on the MI355X against the restatement (tests/huf_util.py), byte for byte; its decoder on its own frames,
on the reference's (tests/golden/huf_streams.npz) and on damaged ones; and, where the compiled reference is present, the
reference's reader on what the device wrote.  The shapes are small: block order 10 makes three chunks of 2 KiB."""
import ctypes as C

import numpy as np
import pytest
import torch

import archive_util as au
import huf_util as hu
from pgrc_amd import HufCoder, PgrcMatchError

pytestmark = pytest.mark.gpu

E_PARAM = 1
LENGTHS = (1, 2, 11, 12, 13, 1023, 1024, 1025, 2048) + tuple(range(2048 + 12 - 3, 2048 + 12 + 5))
ALPHABETS = hu.KINDS + ("one_foreign", "mixed")


@pytest.fixture(scope="module")
def h():
    coder = HufCoder(device=0, block_order=10, table_log=11)
    yield coder
    coder.close()


@pytest.fixture(scope="module")
def ref_decoder():
    return au.ref_decoder() if au.have_ref() else None


def make(kind: str, n: int) -> np.ndarray:
    if kind == "mixed":
        return hu.mixed(n, 10)
    if kind == "one_foreign":                                   # one symbol, and one other byte in the middle chunk only
        x = hu.source("one", n).copy()
        if n > 1024:
            x[min(1500, n - 1)] = 7
        return x
    return hu.source(kind, n)


def at_order(h, order: int, table_log: int = 11):
    h.block_order, h.table_log = order, table_log
    return h


@pytest.mark.parametrize("kind", ALPHABETS)
def test_encode_equals_the_restatement_and_decodes(h, ref_decoder, kind):
    at_order(h, 10)
    for n in LENGTHS:
        x = make(kind, n)
        want = hu.encode(x, 10, 11)
        got = h.encode(x).tobytes()
        assert got == want, (kind, n, len(got), len(want))
        assert h.decode(got, n).tobytes() == x.tobytes(), (kind, n)
        if ref_decoder is not None:
            assert ref_decoder(5, got, n) == x.tobytes(), (kind, n)
    if kind == "uniform":
        assert len(got) > n                                      # every chunk raw: the frame is longer than its source
    t = h.timing()
    assert t["was_decode"] == 1 and t["chunks"] == 3 and t["huf_chunks"] + t["rle_chunks"] + t["raw_chunks"] == 3


def test_an_empty_source_is_the_four_props_bytes(h):
    at_order(h, 10)
    f = h.encode(b"").tobytes()
    assert f == hu.encode(b"", 10, 11) == bytes([0, 10, 255, 11])
    assert h.decode(f, 0).size == 0


@pytest.mark.parametrize("table_log", [8, 9, 10])
def test_other_table_logs_equal_the_restatement(h, table_log):
    at_order(h, 11, table_log)
    for kind in ("fib", "geo", "s130"):
        x = hu.source(kind, 5000)
        got = h.encode(x).tobytes()
        assert got == hu.encode(x, 11, table_log), (kind, table_log)
        assert h.decode(got, x.size).tobytes() == x.tobytes()


def test_the_references_frames_decode(h):
    """the reference's own FSE-coded headers, its code lengths, table log 12"""
    cases = hu.load_golden()
    assert len(cases) >= 8 and any(tl == 12 for _, _, tl, _, _ in cases)
    for name, order, tl, src, frame in cases:
        assert h.decode(frame, src.size).tobytes() == src.tobytes(), name


def test_a_table_log_12_stream_of_the_restatement_decodes(h):
    x = hu.source("fib", 6000)
    chunks = [hu.encode_chunk(c, 12) for c in hu.split(x, 12)]
    assert max(hu.read_stats(c)[1] for c in chunks if 1 < len(c) < 4096) == 12
    f = hu.frame(chunks, 12, 12)
    assert h.decode(f, x.size).tobytes() == x.tobytes()


def test_host_and_device_buffers_at_every_alignment(h):
    at_order(h, 10)
    x = hu.mixed(2048 + 613, 10, seed=9)
    want = hu.encode(x, 10, 11)
    dev = torch.empty(8192, dtype=torch.uint8, device="cuda")
    host_src, host_out = np.empty(8192, np.uint8), np.empty(8192, np.uint8)
    for sa in range(8):
        for oa in range(8):
            s = dev[sa:sa + x.size]
            s.copy_(torch.from_numpy(x))
            o = dev[4096 + oa:4096 + oa + len(want) + 3]
            got = h.encode(s, out=o)
            assert got.is_cuda and got.cpu().numpy().tobytes() == want, (sa, oa)
            back = h.decode(got, x.size, out=dev[sa:sa + x.size].zero_())
            assert back.cpu().numpy().tobytes() == x.tobytes(), (sa, oa)
            host_src[sa:sa + x.size] = x
            got = h.encode(host_src[sa:sa + x.size], out=host_out[oa:oa + len(want)])
            assert got.tobytes() == want, (sa, oa)
            assert h.decode(got, x.size, out=host_src[4096 + oa:4096 + oa + x.size]).tobytes() == x.tobytes()
    # a device source into a host output and back
    assert h.encode(dev[3:3 + x.size].copy_(torch.from_numpy(x)), out=host_out[:len(want)]).tobytes() == want
    assert h.decode(want, x.size, out=dev[5:5 + x.size]).cpu().numpy().tobytes() == x.tobytes()


def test_a_short_output_returns_the_needed_length_and_leaves_the_handle_usable(h):
    from pgrc_amd._lib import hlib
    at_order(h, 10)
    x = hu.mixed(3000, 10)
    want = hu.encode(x, 10, 11)
    out = np.full(len(want) + 8, 0xEE, np.uint8)
    n = C.c_uint64(0)
    rc = hlib.pgrc_huf_encode(h._h, x.ctypes.data, x.size, 0, 10, 11, out.ctypes.data, len(want) - 1, 0, C.byref(n))
    assert rc == E_PARAM and n.value == len(want) and (out == 0xEE).all()
    assert b"below the coded length" in hlib.pgrc_huf_last_error(h._h)
    assert h.encode(x).tobytes() == want


def test_out_of_range_arguments_are_refused(h):
    from pgrc_amd._lib import hlib
    x = hu.source("four", 100)
    out = np.empty(256, np.uint8)
    n = C.c_uint64(0)
    for order, tl in ((0, 11), (18, 11), (10, 12), (10, 7)):
        assert hlib.pgrc_huf_encode(h._h, x.ctypes.data, x.size, 0, order, tl, out.ctypes.data, out.size, 0, C.byref(n)) == E_PARAM
        assert hlib.pgrc_huf_last_error(h._h)
    assert hlib.pgrc_huf_encode(h._h, None, 5, 0, 10, 11, out.ctypes.data, out.size, 0, C.byref(n)) == E_PARAM
    assert hlib.pgrc_huf_encode(h._h, x.ctypes.data, x.size, 0, 10, 11, None, 5, 0, C.byref(n)) == E_PARAM
    assert hlib.pgrc_huf_encode(h._h, x.ctypes.data, x.size, 0, 10, 11, out.ctypes.data, out.size, 0, None) == E_PARAM
    assert hlib.pgrc_huf_decode(h._h, None, 10, 0, 5, out.ctypes.data, 0) == E_PARAM
    assert at_order(h, 10).encode(x).tobytes() == hu.encode(x, 10, 11)


# ---------------------------------------------------------------------------------------------------- damaged input
def damaged_frames():
    """(what, frame, expected_len, a word of the message).  Every case is one the reader refuses from the frame's sizes and the
    chunk's header alone, before any stream is read -- or, for the streams, by the count of bits, which never leaves the
    stream's bytes."""
    x = hu.source("s129", 3 * 2048, seed=6)                    # highest symbol 128: the weights stand raw in the header
    chunks = [hu.encode_chunk(c, 11) for c in hu.split(x, DAMAGED_ORDER)]
    assert all(1 < len(c) < 2048 for c in chunks)
    good = hu.frame(chunks, DAMAGED_ORDER, 11)
    n = x.size
    hs = hu.read_stats(chunks[1])[2]                           # the middle chunk's header bytes
    c1 = 4 + 4 + len(chunks[0]) + 4                            # where the middle chunk starts
    out = [("mode byte 1", bytes([1]) + good[1:], n, "FSE mode"), ("order 18", bytes([0, 18]) + good[2:], n, "above 17"),
           ("mode byte 2", bytes([2]) + good[1:], n, "mode"),
           ("cut inside the props", good[:3], n, "props"), ("cut inside the first size", good[:6], n, "too short"),
           ("cut inside the first chunk", good[:8 + len(chunks[0]) // 2], n, "size"),
           ("cut inside the second size", good[:8 + len(chunks[0]) + 2], n, "size"),
           ("cut inside the last chunk's header", good[:c1 + len(chunks[1]) + 3], n, "chunk 2"),
           ("cut behind the second size", good[:c1], n, "size"), ("cut behind the second chunk", good[:c1 + len(chunks[1])], n, ""),
           ("a chunk size past the end", good[:4] + (len(good)).to_bytes(4, "little") + good[8:], n, "size"),
           ("a chunk size of 0", good[:4] + bytes(4) + good[8:], n, "size"),
           ("a chunk size above the chunk", good[:4] + (2049).to_bytes(4, "little") + good[8:], n, "size")]

    def with_chunk1(c):
        return hu.frame([chunks[0], c, chunks[2]], DAMAGED_ORDER, 11)
    c = bytearray(chunks[1])
    c[hs:hs + 2] = (len(c)).to_bytes(2, "little")
    out.append(("a jump table beyond the chunk", with_chunk1(bytes(c)), n, "jump table"))
    c = bytearray(chunks[1])
    c[1] = (c[1] & 0x0F) | ((((c[1] >> 4) % 11) + 1) << 4)     # another weight for symbol 0: the sum is no power of two
    out.append(("a weight sum that is no power of two", with_chunk1(bytes(c)), n, "weight"))
    size0 = int.from_bytes(chunks[1][hs:hs + 2], "little")
    end0 = hs + 6 + size0 - 1                                  # stream 0's last byte
    # a byte more, or less, at the LOW end of stream 0: the symbols decode as before from the end mark down and then find
    # eight bits left over, or eight too few.  (A change at a stream's high end, such as a frame cut by its last byte, is
    # not a case: a Huffman parse may fall back into step and end where it must, in this reader and in the reference's.)
    c = chunks[1][:hs] + (size0 + 1).to_bytes(2, "little") + chunks[1][hs + 2:hs + 6] + b"\x00" + chunks[1][hs + 6:]
    out.append(("a stream that ends late", with_chunk1(c), n, "early or late"))
    c = chunks[1][:hs] + (size0 - 1).to_bytes(2, "little") + chunks[1][hs + 2:hs + 6] + chunks[1][hs + 7:]
    out.append(("a stream that ends early", with_chunk1(c), n, "early or late"))
    c = bytearray(chunks[1])
    c[end0] = 0
    out.append(("a stream without its end mark", with_chunk1(bytes(c)), n, "end mark"))
    return out, x


DAMAGED_ORDER = 11
DAMAGED, DAMAGED_SRC = damaged_frames()


@pytest.mark.parametrize("case", range(len(DAMAGED)), ids=[d[0].replace(" ", "_") for d in DAMAGED])
def test_damaged_input_is_refused_with_a_message(h, case):
    what, frame, n, word = DAMAGED[case]
    with pytest.raises(hu.HufError):
        hu.decode(frame, n)                                      # (the restatement refuses it too)
    guard = 64
    dev = torch.full((n + 2 * guard,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(PgrcMatchError) as e:
        h.decode(torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).cuda(), n, out=dev[guard:guard + n])
    assert e.value.code == E_PARAM and word in str(e.value) and len(str(e.value)) > 30, (what, str(e.value))
    back = dev.cpu().numpy()
    assert (back[:guard] == 0xEE).all() and (back[guard + n:] == 0xEE).all(), what
    host = np.full(n + guard, 0xEE, np.uint8)
    with pytest.raises(PgrcMatchError):
        h.decode(frame, n, out=host[:n])
    assert (host == 0xEE).all(), what                            # to a host output nothing at all
    x = DAMAGED_SRC
    assert h.decode(at_order(h, DAMAGED_ORDER).encode(x), n).tobytes() == x.tobytes()     # the handle is still good


# ---------------------------------------------------------------------------------------------------- one larger case
def test_eight_mebibytes_device_to_device(h):
    """64 chunks at order 17, the alphabets in turn: the scan over the chunks' sizes and the compaction"""
    at_order(h, 17)
    x = hu.mixed(8 << 20, 17, seed=3)
    want = hu.encode(x, 17, 11)
    src = torch.from_numpy(x).cuda()
    got = h.encode(src)
    assert got.is_cuda and got.cpu().numpy().tobytes() == want
    t = h.timing()
    assert t["chunks"] == 64 and t["huf_chunks"] >= 40 and t["rle_chunks"] == 8 and t["raw_chunks"] == 8 and t["coded_bytes"] == len(want)
    back = h.decode(got, x.size)
    assert back.is_cuda and torch.equal(back, src)
