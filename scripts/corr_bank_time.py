"""Time srcdsp_corr_step_batched against the loop of srcdsp_corr_step over the
same handles.  One process per run, device-resident data, 100 warm-up rounds,
mean of 200 timed rounds.  A correlator step returns its answer to the host, so
the figure is wall-clock time per call (the call's own synchronise included),
taken between two device synchronisations.  Every round runs the batched call
and the loop on fresh clones of the same primed handles (cloned outside the
timed span), so every round scans the same state; the batched call and the loop
alternate, and the loop is timed twice per round so its own run-to-run spread is
on record.  Before timing, the two paths must agree on detections, registers
and bitSamples.  Needs a GPU (no fallback).

Shapes, all at N = 1024, S = 1, noise +-125: (a) 64 channels x 16 384 samples,
no hit; (b) the same with the pattern x 2 at 3/4 of every channel; (c) 8 channels
x 2^22 samples, no hit; (d) one shared input of 2^22 samples, 8 patterns.

Results are merged into the output file shape by shape, so each shape can run
as a process of its own under its own time limit:
  for s in a b c d; do timeout -k 10 600 python scripts/corr_bank_time.py --shapes $s || break; done

Usage: python scripts/corr_bank_time.py [--out profiles/corr_bank_time.json] [--shapes abcd]
       [--warmup 100] [--steps 200]"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import srcdsp_amd as S
from srcdsp_amd.design import qpsk_pattern

N = 1024
SHAPES = {
    "a": dict(name="independent 64ch x 16384, no hit", shared=False, n=1 << 14, C=64, burst=False),
    "b": dict(name="independent 64ch x 16384, burst at 3/4", shared=False, n=1 << 14, C=64, burst=True),
    "c": dict(name="independent 8ch x 2^22, no hit", shared=False, n=1 << 22, C=8, burst=False),
    "d": dict(name="shared 2^22 x 8 patterns, no hit", shared=True, n=1 << 22, C=8, burst=False),
}


def measure(key, shape, warmup, steps):
    C, n, shared = shape["C"], shape["n"], shape["shared"]
    g = torch.Generator(device="cuda").manual_seed(ord(key))
    x = torch.randint(-125, 126, ((n, 2) if shared else (C, n, 2)), dtype=torch.int16, device="cuda", generator=g)
    pats = [qpsk_pattern(N, 500, seed=c + 1) for c in range(C)]
    if shape["burst"]:
        off = (3 * n) // 4
        for c in range(C):
            x[c, off:off + N] += torch.from_numpy((2 * pats[c]).astype(np.int16)).cuda()
    primed = []
    halo = torch.randint(-125, 126, (4096, 2), dtype=torch.int16, device="cuda", generator=g)
    for c in range(C):
        h = S.FixedPatternCorrelator(N, 1)
        h.setPattern(pats[c])
        h.prime(halo)
        primed.append(h)
    rows = [x if shared else x[c] for c in range(C)]

    def clones():
        return [copy.copy(h) for h in primed]

    def batched(hs):
        return S.corr_step_batched(hs, x)

    def loop(hs):
        return [hs[c].step(rows[c]) for c in range(C)]

    # the same step from the same state through both paths
    hb, hl = clones(), clones()
    b0, l0 = S.corr_batched_stats()
    rb = batched(hb)
    b1, l1 = S.corr_batched_stats()
    rl = loop(hl)
    for c in range(C):
        same = (rb[c][0] == rl[c][0] and (not rb[c][0] or rb[c][1] == rl[c][1]) and
                hb[c].getStatus() == hl[c].getStatus() and
                np.array_equal(hb[c].getRefBitSamples(), hl[c].getRefBitSamples()))
        if not same:
            raise SystemExit(f"shape {key}: the batched call and the loop disagree on channel {c}")
    hits = sum(r[0] for r in rb)
    if hits != (C if shape["burst"] else 0):
        raise SystemExit(f"shape {key}: {hits} detections, not what the signal was built for")
    path = "bank kernel" if b1 - b0 == 1 else "per-channel loop"

    names = ("batched", "loop", "loop_again")
    fns = (batched, loop, loop)
    t = {k: [] for k in names}
    for i in range(warmup + steps):
        sets = [clones() for _ in names]
        for k, fn, hs in zip(names, fns, sets):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(hs)
            torch.cuda.synchronize()
            if i >= warmup:
                t[k].append(time.perf_counter() - t0)
    ms = {k: 1e3 * float(np.mean(v)) for k, v in t.items()}
    r = {
        "shape": shape["name"], "channels": C, "samples_per_channel": n, "N": N, "S": 1, "detections": hits,
        "batched_path": path,
        "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
        "loop_spread_ms": round(abs(ms["loop"] - ms["loop_again"]), 5),
        "batched_over_loop": round(ms["batched"] / min(ms["loop"], ms["loop_again"]), 4),
    }
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_bank_time.json"))
    ap.add_argument("--shapes", default="abcd")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corr_bank_time.py needs a GPU")
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
                "protocol": "wall clock per call between device synchronisations, fresh clones of primed handles "
                            "per round; batched, loop, loop alternate per round; means"})
    res.setdefault("results", {})
    for k in a.shapes:
        res["results"][k] = measure(k, SHAPES[k], a.warmup, a.steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
