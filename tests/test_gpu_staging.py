"""stagectx.h's staged copies driven directly (libpgrc_selftest.so): a host buffer goes up with dec_upload_host and comes back
with dec_download_host on a stage of its own, and must come back byte for byte.  The sizes lie around the staging chunk S
(DEC_STAGE_BYTES, asked of the library): below S one chunk, S + 1 the first reuse, 2 S + 5 three chunks -- both staging buffers
are reused on the way up and stage[0] twice on the way down.  Page-locked memory on either side takes the direct copy.  The
fill has no period that divides S, so a chunk that lands at another chunk's offset cannot compare equal."""
import functools

import numpy as np
import pytest

import prim_util as pu

pytestmark = pytest.mark.gpu

# (chunks, bytes beyond them): n = chunks * S + more
SIZES = [(0, 0), (0, 1), (0, 4097), (1, -1), (1, 0), (1, 1), (2, 5)]


@pytest.fixture(scope="module")
def st():
    s = pu.SelfTest(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=1)
def pattern():
    """the longest input; every case takes a prefix of it"""
    a = np.random.default_rng(20241).integers(0, 256, 2 * pu.stage_bytes() + 5, dtype=np.uint8)
    a.setflags(write=False)
    return a


def roundtrip(st, size, pinned_up, pinned_down):
    n = size[0] * pu.stage_bytes() + size[1]
    x = pattern()[:n]
    out, guards = st.stage_roundtrip(x, pinned_up, pinned_down)
    what = f"{n} bytes, pinned up {pinned_up}, down {pinned_down}"
    assert guards == 1, f"{what}: the zone after the device buffer was written"
    assert out.size == n
    if not np.array_equal(out, x):
        bad = np.flatnonzero(out != x)
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {bad[0]}: got {out[bad[0]]}, want {x[bad[0]]}")


def test_chunk_is_a_whole_number_of_lines():
    s = pu.stage_bytes()
    assert s > 4097 and s % 16 == 0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}S{s[1]:+d}")
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_roundtrip(st, size, pinned):
    roundtrip(st, size, pinned, pinned)


def test_roundtrip_pageable_up_pinned_down(st):
    roundtrip(st, (2, 5), False, True)
