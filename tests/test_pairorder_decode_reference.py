"""The pair-order decoder as the device runs it (pgrc_pairorder_decode; pgrc_amd/csrc/pairorder.hip), pinned
on the CPU: tests/pairorder_decode_util's restatement -- offsets from flag scans and a segmented sum, the landing with its
word relaxation and batch ring simulated literally, the two tails, every refusal -- gives the reference-made fixtures'
decoded orders and the literal loop's on generated orders, with batches small enough that marks travel through the ring and
through the bitmap; the header, the library and the Python mirror agree on the new entry points.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pairorder_decode_util as pdu
import pairorder_util as po
from test_pairorder_oracle import FIXTURES, case_name, load_case, random_setting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 128                                     # a batch of two words
ORDERS = pdu.generated_orders(SMALL)
NAMES = ("pgrc_pairorder_decode", "pgrc_decode_set_order_pair_order_streams", "pgrc_pairorder_get_decode_timing")


@pytest.mark.parametrize("path", FIXTURES, ids=case_name)
def test_restatement_gives_the_reference_order(path):
    _, st, decoded, _, _ = load_case(path)
    for batch in (64, SMALL, pdu.BATCH):
        got = pdu.decode(st, batch)
        assert got.dtype == decoded.dtype and got.tobytes() == decoded.tobytes(), batch


@pytest.mark.parametrize("name,org", ORDERS, ids=[n for n, _ in ORDERS])
def test_restatement_equals_the_literal_loop_on_generated_orders(name, org):
    for form in po.FORMS:
        st = po.compress_literal(org, form)
        want = po.decompress_literal(st)
        for batch in (64, SMALL) + ((pdu.BATCH,) if org.size < 20000 else ()):
            stats = {}
            got = pdu.decode(st, batch, stats)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (name, form, batch)
            if form != po.COMPLETE_SINGLE_FILE:
                k = po.kinds(st)
                assert (stats["n_near"], stats["n_delta"], stats["n_full"]) == (k["near"], k["delta"], k["full_set"] + k["full_keep"])


def test_the_batch_order_sends_marks_through_the_ring_and_the_bitmap():
    org = dict(ORDERS)["batches"]
    d, _, _ = pdu.offsets(po.compress_literal(org, po.IGNORE))
    assert set(pdu.batch_wishes(SMALL)) <= set(d.tolist())
    assert (d >= 3 * SMALL).sum() >= 6 and ((d >= 64) & (d < 3 * SMALL)).sum() >= 6
    bases = po.decompress_literal(po.compress_literal(org, po.IGNORE))[0::2]
    assert np.unique(bases[d >= 3 * SMALL] // SMALL).size >= 4             # ... from bases in several batches


@pytest.mark.parametrize("block", range(4))
def test_restatement_equals_the_literal_loop_on_random_settings(block):
    for seed in range(25 * block, 25 * block + 25):
        pairs, form, knobs = random_setting(seed)
        st = po.compress_literal(po.make_order(seed, pairs, **knobs), form)
        assert np.array_equal(pdu.decode(st, 64), po.decompress_literal(st)), (seed, pairs, form, knobs)


def test_rounds_of_the_relaxation():
    """a word whose offsets all reach beyond it settles in its first round; in the all-adjacent order a round makes one more
    pair final (its base and its mate), so a word takes its 32 pairs' rounds and the one that finds nothing changed; with
    every offset dd < 64 a round makes dd more pairs final"""
    for dd in (64, 65, 255, 256):
        stats = {}
        org = pdu.constant_offset_order(dd, 3, dd)
        pdu.decode(po.compress_literal(org, po.IGNORE), SMALL, stats)
        assert stats["landing_rounds"] == stats["landing_words"] > 0, dd
    stats = {}
    pdu.decode(po.compress_literal(pdu.adjacent_order(256), po.IGNORE), SMALL, stats)
    assert stats["landing_words"] == 8 and stats["landing_rounds"] == 33 * 8
    for dd, per_word in ((2, 17), (4, 9), (32, 2)):
        stats = {}
        pdu.decode(po.compress_literal(pdu.constant_offset_order(dd, 256 // dd, dd), po.IGNORE), SMALL, stats)
        assert stats["landing_rounds"] == per_word * stats["landing_words"], (dd, stats)
    # the worst word by hand: no order, but offsets that make every round settle one slot only
    M, r, lanes = pdu.settle(0, 0, np.array([1] * 64), 64)
    assert r <= 64 and [j for j, _, _ in lanes] == list(range(0, 64, 2))


def test_settle_is_the_serial_rule_on_random_words():
    rng = np.random.default_rng(5)
    for _ in range(300):
        E = int(rng.integers(0, 1 << 62)) & int(rng.integers(0, 1 << 62))
        d = rng.choice([1, 2, 3, 5, 8, 13, 31, 32, 33, 62, 63, 64, 100], size=64)
        got = pdu.settle(E, 0, d, 64)
        assert got is not None
        M, k = E, 0
        for j in range(64):                     # the reference's walk over the word
            if (M >> j) & 1:
                continue
            if j + d[k] < 64:
                M |= 1 << (j + int(d[k]))
            k += 1
        assert got[0] == M and len(got[2]) == k and got[1] <= 64


CASES = pdu.refusal_cases()


@pytest.mark.parametrize("what,st,names", CASES, ids=[c[0] for c in CASES])
def test_restatement_refuses(what, st, names):
    with pytest.raises(pdu.Refused) as e:
        pdu.decode(st, 64)
    assert names in str(e.value), (what, str(e.value))


def test_library_header_and_mirror_agree_on_the_decoder(tmp_path):
    from pgrc_amd import _lib, decode
    import pgrc_amd
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgrc_pairorder_decode.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(pgrc_\w+)\s*\(", txt)) == set(NAMES)
    assert '#include "pgrc_pairorder_decode.h"' in open(os.path.join(ROOT, "include", "pgrc_decode.h")).read()
    assert f"#define PGRC_PAIRORDER_DECODE_BATCH {decode.PGRC_PAIRORDER_DECODE_BATCH}u" in txt and decode.PGRC_PAIRORDER_DECODE_BATCH == pdu.BATCH
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    protos = {name for name, _, _ in decode.DECODE_PROTOS}
    for s in NAMES:
        assert s in exported and s in protos and getattr(_lib.lib, s).argtypes is not None, s
    assert callable(pgrc_amd.decompressReadsOrder) and callable(pgrc_amd.PgRCDecoder.set_order_pair_order_streams)
    assert callable(pgrc_amd.PgRCDecoder.decompressReadsOrder) and callable(pgrc_amd.PgRCDecoder.pairorder_decode_timing)
    # the timing struct, laid out as the header lays it out (through pgrc_decode.h, as a caller includes it)
    st = _lib.PairOrderDecodeTiming
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pgrc_decode.h"', 'int main(void) {',
             '    printf("%zu\\n", sizeof(pgrc_pairorder_decode_timing));']
    lines += [f'    printf("%zu %zu\\n", offsetof(pgrc_pairorder_decode_timing, {f}), sizeof(((pgrc_pairorder_decode_timing *)0)->{f}));' for f, _ in st._fields_]
    lines += ['    printf("%zu %zu\\n", sizeof(pgrc_pairorder_streams), sizeof(pgrc_pairorder_timing));', '    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = iter(subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"))
    assert int(next(out)) == C.sizeof(st) == 96
    for f, _ in st._fields_:
        assert tuple(int(x) for x in next(out).split()) == (getattr(st, f).offset, getattr(st, f).size), f
    assert next(out).split() == ["120", "80"]                              # the structs that were there did not grow


def test_null_arguments_are_refused_without_a_device():
    from pgrc_amd import _lib
    from pgrc_amd.decode import PairOrderStreams
    lib = _lib.lib
    s, t = PairOrderStreams(), _lib.PairOrderDecodeTiming()
    assert lib.pgrc_pairorder_decode(None, C.byref(s), None) == 1
    assert lib.pgrc_decode_set_order_pair_order_streams(None, C.byref(s), 0) == 1
    assert lib.pgrc_pairorder_get_decode_timing(None, C.byref(t)) == 1
