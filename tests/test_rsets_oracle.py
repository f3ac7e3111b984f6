"""The two restatements of DividedPCLReadsSets' edits in tests/rsets_util.py -- the reference's loops line by line and the
class-per-index form the device uses -- against the fixtures of the compiled reference (tests/golden/rsets_*.npz, made by
tests/golden/make_golden_rsets.py) and against each other on random small settings, empty sets included.  No GPU."""
import glob
import os

import numpy as np
import pytest

import rsets_util as ru

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ru.GOLDEN, "rsets_*.npz")))
FORMS = {"literal": (ru.literal_move, ru.literal_hq_mapping, ru.literal_remove), "class": (ru.class_move, ru.class_hq_mapping, ru.class_remove)}


def test_the_fixtures_cover_what_they_must():
    fx = {n: ru.load_fixture(n) for n in FIXTURES}
    assert {(f["L"], f["separate_n"]) for f in fx.values()} >= {(21, True), (21, False), (150, True), (150, False)}
    assert {f["before"]["hq"].shape[1] for f in fx.values()} >= {6, 7, 38, 50}
    assert {n.split("_")[-1][:-4] for n in FIXTURES} >= {"mixed", "earlyend", "noflag", "allflags", "lqempty", "single"}

    def ends_mixed(part):       # kept and removed rows at both ends
        return part[:2].any() and not part[:2].all() and part[-2:].any() and not part[-2:].all()
    for name in ("rsets_L21_sepN_mixed.npz", "rsets_L150_sepN_mixed.npz"):
        f = fx[name]
        b, flags, g = f["before"], f["is_hq"].astype(bool), f["is_mapped"].astype(bool)
        hq_idx = ru.class_hq_mapping(b)[:-1]
        moved, stays = hq_idx[~flags], hq_idx[flags]
        lq, n = b["lq_map"][:-1], b["n_map"][:-1]
        assert moved.min() < lq.min() and moved.max() > lq.max()            # moved reads below the first and above the last old LQ index
        assert (lq < stays.min()).any()                                     # old LQ entries below the smallest index that stays HQ
        assert ((n > lq.min()) & (n < stays.min())).any() and ((n > lq.max()) & (n < moved.max())).any()   # N entries between them
        nl = f["moved"]["lq"].shape[0]
        assert ends_mixed(g[:nl]) and ends_mixed(g[nl:])
    early = fx["rsets_L150_sepN_earlyend.npz"]["before"]                    # old LQ entries below every HQ index: the loop's early end
    assert early["lq_map"][1] < ru.class_hq_mapping(early)[0]
    assert fx["rsets_L150_sepN_lqempty.npz"]["before"]["lq"].shape[0] == 0 and fx["rsets_L21_plain_single.npz"]["before"]["A"] == 1
    assert not fx["rsets_L21_sepN_noflag.npz"]["is_hq"].any() and fx["rsets_L21_sepN_allflags.npz"]["is_hq"].all()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", FIXTURES)
def test_restatements_equal_the_compiled_reference(name, form):
    move, hq_mapping, remove = FORMS[form]
    f = ru.load_fixture(name)
    m = move(f["before"], f["is_hq"])
    assert ru.same_state(m, f["moved"])
    assert np.array_equal(hq_mapping(m), f["hq_mapping"])
    assert ru.same_state(remove(m, f["is_mapped"]), f["removed"])


def test_the_two_forms_agree_on_random_small_settings():
    rng = np.random.default_rng(2024)
    seen_empty = [False, False, False]
    for t in range(400):
        separate_n = bool(t % 2)
        A = int(rng.integers(0, 61))
        st = ru.random_state(rng, int(rng.choice([1, 21, 150])), separate_n, A, p_lq=float(rng.choice([0, 0.1, 0.4, 1])), p_n=float(rng.choice([0, 0.2, 1])))
        for k, key in enumerate(("hq", "lq", "n")):
            seen_empty[k] |= st[key] is not None and st[key].shape[0] == 0 and A > 0
        cur_l = cur_c = st
        for density in (float(rng.choice([0, 0.5, 1])), 0.5):               # move, and move again
            f = (rng.random(cur_l["hq"].shape[0]) < density).astype(np.uint8)
            cur_l, cur_c = ru.literal_move(cur_l, f), ru.class_move(cur_c, f)
            assert ru.same_state(cur_l, cur_c), (t, density)
            assert np.array_equal(cur_l["lq_map"][:-1], np.sort(cur_l["lq_map"][:-1])) and cur_l["lq_map"][-1] == A
        assert np.array_equal(ru.literal_hq_mapping(cur_l), ru.class_hq_mapping(cur_c))
        g = (rng.random(cur_l["lq"].shape[0] + (cur_l["n"].shape[0] if separate_n else 0)) < float(rng.choice([0, 0.5, 1]))).astype(np.uint8)
        assert ru.same_state(ru.literal_remove(cur_l, g), ru.class_remove(cur_c, g)), t
    assert all(seen_empty)
