"""The shared primitives (scanops.h, radix.hip) against numpy: the ctypes binding of libpgrc_selftest.so and the plain
references of every scan and sort it reaches.  The references are vectorised numpy on 64-bit integers;
tests/test_prim_reference.py holds each of them to a literal loop of its operator on the CPU."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# PGRC_SELFTEST_LIB: another build of the same library (a mutated scratch copy, to see that the tests notice)
LIB_PATH = os.environ.get("PGRC_SELFTEST_LIB") or os.path.join(ROOT, "pgrc_amd", "libpgrc_selftest.so")

GUARD = 64                  # selftest.hip ST_GUARD
FILL = 0xA5                 # selftest.hip ST_FILL
NONE = 0xFFFFFFFF           # mem.hip MR_NONE: the identity of "last valid"
SEG = np.dtype([("v", "<i8"), ("set", "<u4")])      # the 12-byte element of the segmented sum (pairpos.hip PpSeg)
assert SEG.itemsize == 12

# selftest.hip's kinds of the device scan: (number, input type, output type)
U32_SUM_U32, U32_FLAG_U8, U64_SUM_U8, U64_SUM_U16, U64_SUM_U32, U64_SUM_U64, U64_MAX, U32_LAST_VALID, SEG_SUM = range(9)
SCAN_TYPES = {U32_SUM_U32: (np.uint32, np.uint32), U32_FLAG_U8: (np.uint8, np.uint32), U64_SUM_U8: (np.uint8, np.uint64),
              U64_SUM_U16: (np.uint16, np.uint64), U64_SUM_U32: (np.uint32, np.uint64), U64_SUM_U64: (np.uint64, np.uint64),
              U64_MAX: (np.uint64, np.uint64), U32_LAST_VALID: (np.uint32, np.uint32), SEG_SUM: (SEG, SEG)}
# ... and of the block scan
BLK_SUM_U32, BLK_SUM_U64, BLK_MAX_U64, BLK_SEG = range(4)
BLOCK_TYPES = {BLK_SUM_U32: np.uint32, BLK_SUM_U64: np.uint64, BLK_MAX_U64: np.uint64, BLK_SEG: SEG}

SCO_EPB = 4096              # scanops.h: elements per block of the device scan
SCO_ROUND = 256 * SCO_EPB   # ... and per round of its carry kernel
RX_TILE = 8192              # radix.hip: records per tile = the largest segment of the segment sort


# ---------------------------------------------------------------------------------------------- references
def fill_of(dtype, count=1):
    """`count` elements as the entries leave memory they did not write"""
    return np.frombuffer(bytes([FILL]) * (np.dtype(dtype).itemsize * count), dtype=dtype)


def _shift(first, inc):
    """[first, inc[0], ..., inc[n-2]] in inc's type: the exclusive scan from the inclusive one"""
    out = np.empty_like(inc)
    if inc.size:
        out[0] = first
        out[1:] = inc[:-1]
    return out


def ref_sum(x, width, start=0, inclusive=True):
    """the running sum of x in `width` bits, wrapped as the kernel wraps; returns (out[0 .. n), total)"""
    mask = np.uint64((1 << width) - 1)
    s = np.uint64(start & ((1 << width) - 1))
    inc = (np.cumsum(x.astype(np.uint64), dtype=np.uint64) + s) & mask
    total = inc[-1] if x.size else s
    return (inc if inclusive else _shift(s, inc)), total


def ref_max(x, inclusive=True):
    inc = np.maximum.accumulate(x.astype(np.uint64)) if x.size else x.astype(np.uint64)
    return inc if inclusive else _shift(0, inc)


def ref_last_valid(x, inclusive=False):
    """the rightmost value != NONE at or before (inclusive) / before (exclusive) every index, NONE where there is none"""
    x = x.astype(np.uint32)
    if not x.size:
        return x
    idx = np.where(x != NONE, np.arange(x.size, dtype=np.int64), -1)
    last = np.maximum.accumulate(idx)
    inc = np.where(last >= 0, x[np.maximum(last, 0)], NONE).astype(np.uint32)
    return inc if inclusive else _shift(NONE, inc)


def ref_seg_sum(v, flag, inclusive=True):
    """the fold of (a, b) -> b.set ? b : (a.v + b.v, a.set) from (0, 0): the sum since the last element with a flag, and that
    element's flag; from two cumulative sums.  Returns (v, set)."""
    v = v.astype(np.int64)
    flag = flag.astype(np.uint32)
    n = v.size
    if not n:
        return v, flag
    c = np.cumsum(v, dtype=np.int64)
    idx = np.where(flag != 0, np.arange(n, dtype=np.int64), -1)
    last = np.maximum.accumulate(idx)
    at = np.maximum(last, 0)
    before = np.where(last >= 0, c[at] - v[at], 0)          # the sum of everything before the last flagged element
    ov = c - before
    os_ = np.where(last >= 0, flag[at], 0).astype(np.uint32)
    if not inclusive:
        ov, os_ = _shift(0, ov), _shift(0, os_)
    return ov, os_


def seg_pack(v, flag):
    a = np.empty(len(v), dtype=SEG)
    a["v"] = v
    a["set"] = flag
    return a


def seg_op(a, b):
    """the operator itself, element by element over two SEG arrays"""
    with np.errstate(over="ignore"):
        return seg_pack(np.where(b["set"] != 0, b["v"], a["v"] + b["v"]), np.where(b["set"] != 0, b["set"], a["set"]))


def field_of(keys, bit_lo, bit_hi):
    w = bit_hi - bit_lo
    if w <= 0:
        return np.zeros(keys.size, dtype=np.uint64)
    return (keys >> np.uint64(bit_lo)) & np.uint64((1 << w) - 1)


def ref_stable_order(keys, bit_lo, bit_hi):
    """input indexes in the order a stable sort by the bits [bit_lo, bit_hi) leaves them"""
    return np.argsort(field_of(keys, bit_lo, bit_hi), kind="stable")


def rx_split(bits):
    """the digit widths of rx_sort's passes over a field of `bits` bits, lowest digit first (radix.hip: "digits as even as the
    field allows")"""
    passes = (bits + 7) // 8
    out, done = [], 0
    for p in range(passes):
        d = (bits - done + (passes - p) - 1) // (passes - p)
        out.append(d)
        done += d
    return out


def ref_block(kind, x):
    """(exclusive, total, second) of selftest.hip's block kernel: the exclusive scan of x, its total, and the exclusive scan
    of op(first exclusive value, x in reverse thread order)"""
    if kind in (BLK_SUM_U32, BLK_SUM_U64):
        width = 32 if kind == BLK_SUM_U32 else 64
        dt = BLOCK_TYPES[kind]
        ex, tot = ref_sum(x, width, inclusive=False)
        v2 = (ex + x[::-1].astype(np.uint64)) & np.uint64((1 << width) - 1)
        return ex.astype(dt), dt(tot), ref_sum(v2, width, inclusive=False)[0].astype(dt)
    if kind == BLK_MAX_U64:
        ex = ref_max(x, inclusive=False)
        return ex, x.max(), ref_max(np.maximum(ex, x[::-1]), inclusive=False)
    ev, es = ref_seg_sum(x["v"], x["set"], inclusive=False)
    tv, ts = ref_seg_sum(x["v"], x["set"], inclusive=True)
    v2 = seg_op(seg_pack(ev, es), x[::-1])
    return seg_pack(ev, es), seg_pack(tv[-1:], ts[-1:])[0], seg_pack(*ref_seg_sum(v2["v"], v2["set"], inclusive=False))


# ---------------------------------------------------------------------------------------------- the library
_lib = None


def lib():
    global _lib
    if _lib is None:
        from pgrc_amd import _lib as product  # noqa: F401  (loads the process's one HIP runtime first)
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: `make -C pgrc_amd/csrc` builds it beside libpgrc_match.so")
        L = C.CDLL(LIB_PATH)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        L.pgrc_selftest_create.argtypes = [i32, C.POINTER(vp)]
        L.pgrc_selftest_destroy.argtypes = [vp]
        L.pgrc_selftest_destroy.restype = None
        L.pgrc_selftest_last_error.argtypes = [vp]
        L.pgrc_selftest_last_error.restype = C.c_char_p
        L.pgrc_selftest_scratch_elems.argtypes = [u64]
        L.pgrc_selftest_scratch_elems.restype = u64
        L.pgrc_selftest_device_scan.argtypes = [vp, i32, vp, u64, u64, i32, i32, i32, vp, C.POINTER(u32)]
        L.pgrc_selftest_block_scan.argtypes = [vp, i32, u32, i32, i32, vp, vp, vp, vp, C.POINTER(u32)]
        L.pgrc_selftest_sort.argtypes = [vp, vp, vp, u64, u32, u32, vp, vp, C.POINTER(u32)]
        L.pgrc_selftest_sort_segments.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp, C.POINTER(u32)]
        L.pgrc_selftest_stage_bytes.argtypes = []
        L.pgrc_selftest_stage_bytes.restype = u64
        L.pgrc_selftest_stage_roundtrip.argtypes = [vp, vp, u64, i32, i32, vp, C.POINTER(u32)]
        _lib = L
    return _lib


def stage_bytes():
    """stagectx.h DEC_STAGE_BYTES: the staging chunk of the copies between pageable host memory and the device"""
    return lib().pgrc_selftest_stage_bytes()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class SelfTest:
    """one context: a device, a stream and the sort's scratch"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        e = lib().pgrc_selftest_create(device, C.byref(self.h))
        if e:
            raise RuntimeError(f"pgrc_selftest_create: error {e}")

    def close(self):
        if self.h:
            lib().pgrc_selftest_destroy(self.h)
            self.h = C.c_void_p()

    def _check(self, e, what):
        if e:
            raise RuntimeError(f"{what}: error {e}: {lib().pgrc_selftest_last_error(self.h).decode()}")

    def device_scan(self, kind, x, start=0, inclusive=True, total_at_n=False, in_place=False):
        """-> (out[0 .. n], guards): n + 1 elements, the last one FILL bytes unless a total was written; guards == 3: intact"""
        tin, tout = SCAN_TYPES[kind]
        x = np.ascontiguousarray(x, dtype=tin)
        out = np.zeros(x.size + 1, dtype=tout)
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_device_scan(self.h, kind, _ptr(x), x.size, start, int(inclusive), int(total_at_n), int(in_place), _ptr(out), C.byref(g)),
                    "device_scan")
        return out, g.value

    def block_scan(self, kind, x, nwv_static, sync_after):
        """-> (exclusive, total per thread, second, guards); guards == 7: intact"""
        dt = BLOCK_TYPES[kind]
        x = np.ascontiguousarray(x, dtype=dt)
        outs = [np.zeros(x.size, dtype=dt) for _ in range(3)]
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_block_scan(self.h, kind, x.size, int(nwv_static), int(sync_after), _ptr(x), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                                   C.byref(g)), "block_scan")
        return outs[0], outs[1], outs[2], g.value

    def sort(self, keys, vals, bit_lo, bit_hi):
        """-> (keys, values or None, guards); guards == 15: intact"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        ok = np.zeros(keys.size, dtype=np.uint64)
        ov = None
        if vals is not None:
            vals = np.ascontiguousarray(vals, dtype=np.uint64)
            ov = np.zeros(keys.size, dtype=np.uint64)
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_sort(self.h, _ptr(keys), _ptr(vals) if vals is not None else None, keys.size, bit_lo, bit_hi, _ptr(ok),
                                             _ptr(ov) if ov is not None else None, C.byref(g)), "sort")
        return ok, ov, g.value

    def stage_roundtrip(self, x, pinned_up, pinned_down):
        """x up and down again through a stage; each side page-locked or pageable -> (the bytes that came back, guards); guards == 1: intact"""
        x = np.ascontiguousarray(x, dtype=np.uint8)
        out = np.zeros(x.size, dtype=np.uint8)
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_stage_roundtrip(self.h, _ptr(x), x.size, int(pinned_up), int(pinned_down), _ptr(out), C.byref(g)), "stage_roundtrip")
        return out, g.value

    def sort_segments(self, keys, vals, seg, bit_lo, bit_hi, top_bits, cap):
        """-> (keys, values, ovl[0 .. cap], guards); guards == 7: intact"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        seg = np.ascontiguousarray(seg, dtype=np.uint32)
        assert seg[-1] == keys.size == vals.size
        ok, ov, ovl = np.zeros(keys.size, dtype=np.uint64), np.zeros(keys.size, dtype=np.uint64), np.zeros(cap + 1, dtype=np.uint32)
        g = C.c_uint32(0)
        self._check(lib().pgrc_selftest_sort_segments(self.h, _ptr(keys), _ptr(vals), _ptr(seg), seg.size - 1, bit_lo, bit_hi, top_bits, cap, _ptr(ok), _ptr(ov),
                                                      _ptr(ovl), C.byref(g)), "sort_segments")
        return ok, ov, ovl, g.value
