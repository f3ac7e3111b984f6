"""Rate of the variable-length DNA coder on the device and of the two stages that use it.

The inputs of tools/pgmap_rate.py at C3 size: a synthetic 1.875 Gbp HQ with planted reverse-complement copies and a 60 Mbp
LQ.  In one process, per direction, the path that moves the mapped text at one byte a symbol against the one that moves it
coded:

  encoder   markAndRemoveExactMatches (LQ, HQ: the mapped text downloaded)  against  markAndRemoveExactMatchesResident (LQ,
            HQ) + encodeMapped (the coded bytes downloaded), into pageable and into page-locked memory
  decoder   restoreMatchedPgs (the mapped text uploaded)  against  set_mapped_text_coded (the coded bytes uploaded), from
            pageable and from page-locked memory

with the coder's device time by phase, the coded ratio of that text, and the check that both decoder paths install texts
with the originals' digests.  Whole calls are host-clock times of five repeats after a warm-up (median, min, max).  The book
is the encoder's (id 0), read from a recorded stream under tests/golden.  Prints one JSON line.

    python tools/varlen_rate.py [--pg-len G] [--lq-len N] [--out profiles/varlen_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pgmap_util as pu  # noqa: E402
import varlen_util as vu  # noqa: E402
from pgmap_rate import REPEATS, spread  # noqa: E402
from restore_rate import digest, plant  # noqa: E402

CODER_PHASES = ("ms_upload", "ms_maps", "ms_scan", "ms_emit", "ms_download", "ms_call")


def timed(fn):
    """a warm-up, then REPEATS calls -> (the last result, the calls' ms)"""
    res = fn()
    ms = []
    for _ in range(REPEATS):
        c0 = time.perf_counter()
        res = fn()
        ms.append((time.perf_counter() - c0) * 1e3)
    return res, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pg-len", type=int, default=1_875_000_000)
    ap.add_argument("--lq-len", type=int, default=60_000_000)
    ap.add_argument("--target-len", type=int, default=45)
    ap.add_argument("--copies", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pgrc_amd import CopMEMMatcher, PgRCDecoder, VarLenDNACoder, synth

    t0 = time.time()
    G, GL, tl = args.pg_len, args.lq_len, args.target_len
    hq = synth.pg_host(synth.pg_params(G, seed=77, tandem_every=64))
    rng = np.random.default_rng(77)
    plant(hq, rng, args.copies, 3)
    lq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=GL)
    for _ in range(GL // 3000):
        ln = int(rng.integers(100, 2000))
        s, d = int(rng.integers(0, G - ln)), int(rng.integers(0, GL - ln))
        lq[d:d + ln] = pu.revcomp_np(hq[s:s + ln]) if rng.random() < 0.7 else hq[s:s + ln]
    t_gen = time.time() - t0
    want = {"hq": digest(hq), "lq": digest(lq)}

    book = next(vu.parse_stream(streams[0])[2] for _, _, streams in vu.load_fixtures() if 0 in streams)
    coder = VarLenDNACoder(book.raw + b"\0", device=0)
    tm = CopMEMMatcher(hq, tl, device=0)
    pageable = np.empty(G, dtype=np.uint8)
    pinned = torch.empty(G, dtype=torch.uint8).pin_memory().numpy()
    parts, enc = {}, {}
    for name, dest, dis, slot in (("lq", lq, False, 1), ("hq", hq, True, 0)):
        found = tm.matchTexts(pu.revcomp_np(dest), dis, True)
        res_page, ms_page = timed(lambda: tm.markAndRemoveExactMatches(found, None, pageable[:dest.size]))
        res_pin, ms_pin = timed(lambda: tm.markAndRemoveExactMatches(found, None, pinned[:dest.size]))
        res_res, ms_res = timed(lambda: tm.markAndRemoveExactMatchesResident(found, slot))
        mapped, off, lens, info = res_pin
        assert res_res[0] == mapped.size and res_res[1].tobytes() == off.tobytes() and res_res[2].tobytes() == lens.tobytes()
        parts[name] = (mapped.tobytes(), off.tobytes(), lens.tobytes())
        enc[name] = {"dest_len": int(dest.size), "marks": int(info["marks"]), "mapped_len": int(mapped.size),
                     "mark_and_remove_call_ms_pageable": spread(ms_page), "mark_and_remove_call_ms_pinned": spread(ms_pin),
                     "mark_and_remove_resident_call_ms": spread(ms_res)}
    mapped, mlens, offs, lns = pu.join_parts([parts["hq"], parts["lq"], (b"", b"", b"")])
    mapped = np.frombuffer(mapped, np.uint8)
    bound = VarLenDNACoder.bound(mapped.size)
    coded_page = np.empty(bound, dtype=np.uint8)
    coded_pin = torch.empty(bound, dtype=torch.uint8).pin_memory().numpy()
    (coded, lens3), ms_code_page = timed(lambda: tm.encodeMapped(coder, coded_page))
    (coded_p, _), ms_code_pin = timed(lambda: tm.encodeMapped(coder, coded_pin))
    enc_phases = coder.timing()
    assert coded.tobytes() == coded_p.tobytes() and list(lens3) == mlens
    coded = coded_p.copy()
    tm.close()
    med = lambda d: d["median"]  # noqa: E731
    enc["encode_mapped_call_ms_pageable"] = spread(ms_code_page)
    enc["encode_mapped_call_ms_pinned"] = spread(ms_code_pin)
    enc["coder_ms_last_encode"] = {k: round(float(enc_phases[k]), 3) for k in CODER_PHASES}
    for mem in ("pageable", "pinned"):
        enc[f"sum_text_downloaded_ms_{mem}"] = round(sum(med(enc[p][f"mark_and_remove_call_ms_{mem}"]) for p in ("lq", "hq")), 3)
        enc[f"sum_coded_downloaded_ms_{mem}"] = round(sum(med(enc[p]["mark_and_remove_resident_call_ms"]) for p in ("lq", "hq"))
                                                      + med(enc[f"encode_mapped_call_ms_{mem}"]), 3)

    # the coder alone, device to device, on the joined mapped text
    d_text = torch.from_numpy(mapped).cuda()
    d_out = torch.empty(coded.size, dtype=torch.uint8, device="cuda")
    d_coded, _ = timed(lambda: coder.encode(d_text, out=d_out))
    dd_enc = coder.timing()
    assert d_coded.cpu().numpy().tobytes() == coded.tobytes()
    d_back, _ = timed(lambda: coder.decode(d_coded, mapped.size, out=d_text))
    dd_dec = coder.timing()
    assert digest(d_back.cpu().numpy()) == digest(mapped)
    del d_text, d_out, d_coded, d_back

    dec = PgRCDecoder(150, device=0)
    mapped_pin = torch.empty(mapped.size, dtype=torch.uint8).pin_memory().numpy()
    mapped_pin[:] = mapped
    coded_pin[:coded.size] = coded
    _, ms_plain = timed(lambda: dec.restoreMatchedPgs(mapped, mlens, G, offs, lns))
    _, ms_plain_pin = timed(lambda: dec.restoreMatchedPgs(mapped_pin, mlens, G, offs, lns))
    rt_plain = dec.restore_timing()
    out = dec.text()
    got_plain = {"hq": digest(out[:G]), "lq": digest(out[G:])}
    _, ms_coded_pin = timed(lambda: dec.set_mapped_text_coded(coder, coded_pin[:coded.size], mlens, G, offs, lns))
    _, ms_coded = timed(lambda: dec.set_mapped_text_coded(coder, coded, mlens, G, offs, lns))
    dec_phases = coder.timing()
    rt = dec.restore_timing()
    out = dec.text()
    got_coded = {"hq": digest(out[:G]), "lq": digest(out[G:])}
    dec.close()
    coder.close()

    res = {
        "what": "the variable-length DNA coder on the device at C3 size: the mapped text moved as bytes against moved coded, both directions, one process",
        "pg_len": G, "lq_len": GL, "target_len": tl, "copies_planted": args.copies, "repeats": REPEATS, "book_id": 0,
        "mapped_symbols": int(mapped.size), "coded_bytes": int(coded.size), "coded_ratio": round(coded.size / mapped.size, 4),
        "encoder": enc,
        "coder_device_to_device_ms": {"encode": {k: round(float(dd_enc[k]), 3) for k in CODER_PHASES},
                                      "decode": {k: round(float(dd_dec[k]), 3) for k in CODER_PHASES}},
        "decoder": {"set_mapped_text_call_ms_pageable": spread(ms_plain), "set_mapped_text_call_ms_pinned": spread(ms_plain_pin),
                    "set_mapped_text_coded_call_ms_pageable": spread(ms_coded), "set_mapped_text_coded_call_ms_pinned": spread(ms_coded_pin),
                    "restore_timing_last_plain_pinned": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rt_plain.items()},
                    "coder_ms_last_decode": {k: round(float(dec_phases[k]), 3) for k in CODER_PHASES},
                    "restore_timing_last_coded": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rt.items()}},
        "round_trip": {"digest_want": want, "digest_got_plain": got_plain, "digest_got_coded": got_coded,
                       "equal": want == got_plain == got_coded},
        "host_generate_s": round(t_gen, 1),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["round_trip"]["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
