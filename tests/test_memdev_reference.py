"""tests/memdev_util.py's numpy reference of the device-side packing (mempack.hip) against what exists already: the reversed
form equals the forward form of oracle.revcomp_ascii's text -- what the host route packs --, the forward form equals
handover_util's text packer and a literal loop over the symbols, with N's and with a byte outside ACGNT; the pad is zero.
No GPU."""
import subprocess

import numpy as np
import pytest

import handover_util as hu
import memdev_util as mu
import oracle as orc

LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 45, 255, 256, 257, 4095, 4096, 4097, 8197]


def texts(n, seed):
    """(name, text): clean; N's at both ends, across a word boundary and at random; the same with one bad byte"""
    rng = np.random.default_rng(seed)
    clean = mu.random_text(n, seed)
    with_n = mu.random_text(n, seed + 1, n_at=[0, n - 1, 15, 16] + rng.integers(0, n, size=max(1, n // 50)).tolist())
    bad = with_n.copy()
    bad[int(rng.integers(0, n))] = ord("%")
    return [("clean", clean), ("n", with_n), ("bad", bad)]


@pytest.mark.parametrize("n", LENGTHS)
def test_reversed_packing_is_the_forward_packing_of_the_host_reversed_text(n):
    for name, t in texts(n, 3 * n):
        fw = mu.pack_ref(orc.revcomp_ascii(t), False)
        rv = mu.pack_ref(t, True)
        assert rv[2] == fw[2] == (1 if name == "bad" else 0) | (2 if (t == mu.N).any() else 0), (n, name)
        assert np.array_equal(rv[0], fw[0]) and np.array_equal(rv[1], fw[1]), (n, name)


@pytest.mark.parametrize("n", LENGTHS)
def test_forward_packing_equals_the_text_packer_and_a_literal_loop(n):
    for name, t in texts(n, 5 * n + 1):
        words, nmap, flags = mu.pack_ref(t, False)
        nwords = (n + 15) // 16
        assert words.size == nmap.size == nwords + mu.PAD_WORDS
        assert not words[nwords:].any() and not nmap[nwords:].any(), "the pad words are zero"
        if n % 16:
            assert words[nwords - 1] >> np.uint32(2 * (n % 16)) == 0 and nmap[nwords - 1] >> np.uint16(n % 16) == 0, "zero above the last symbol"
        if name == "clean":
            assert flags == 0 and not nmap.any()
            assert np.array_equal(words[:nwords], hu.pack_text(t))
        want_w, want_n, want_f = np.zeros(nwords, np.uint32), np.zeros(nwords, np.uint16), 0
        for i, ch in enumerate(t.tolist()):
            if ch == mu.N:
                want_n[i // 16] |= np.uint16(1 << (i % 16))
                want_f |= 2
            elif ch in b"ACGT":
                want_w[i // 16] |= np.uint32(b"ACGT".index(ch) << (2 * (i % 16)))
            else:
                want_f |= 1
        assert flags == want_f, (n, name)
        assert np.array_equal(words[:nwords], want_w) and np.array_equal(nmap[:nwords], want_n), (n, name)


def test_the_n_map_marks_the_byte_the_symbol_came_from():
    """reversed, output symbol i is input byte n - 1 - i, an N there is an N here and packs as code 0, not as its 'complement'"""
    t = np.frombuffer(b"ACGTNACGTTTTTTTTTAN", dtype=np.uint8)            # 19 symbols
    words, nmap, flags = mu.pack_ref(t, True)
    back = orc.revcomp_ascii(t)
    assert back.tobytes() == b"NTAAAAAAAAACGTNACGT"
    assert flags == 2 and nmap[0] == (1 << 0) | (1 << 14) and nmap[1] == 0
    sym = [(int(words[i // 16]) >> (2 * (i % 16))) & 3 for i in range(19)]
    assert sym == [0 if ch == mu.N else b"ACGT".index(ch) for ch in back.tolist()]


def test_the_selftest_entry_stays_out_of_the_product_library():
    from pgrc_amd import _lib
    import prim_util as pu

    def names(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "pgrc_selftest_mem_pack_device" in names(pu.LIB_PATH)
    assert "pgrc_selftest_mem_pack_device" not in names(_lib.LIB_PATH)
