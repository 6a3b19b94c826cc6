"""Time srcdsp_corr_step_all against the loops it replaces.  The protocol of
scripts/corr_bank_time.py: one process, device-resident data, warm-up rounds,
then the mean of the timed rounds of wall-clock time per call between two
device synchronisations; every round runs every alternative on fresh clones of
the same primed handles (cloned outside the timed span); the alternatives
alternate and each is timed twice per round, so its own run-to-run spread is on
record.  Before timing, the alternatives must agree on detections, registers
and bitSamples.  Needs a GPU (no fallback).

Shapes, all at N = 1024, S = 1, noise +-125, bursts = the pattern x 2, evenly
spaced:
 (a) 64 channels x 16 384 samples, 4 bursts each: the new call against the host
     loop of corr_step_batched on the remainders and the loop of single steps;
 (b) one row of 2^22 samples, 64 bursts, against the loop of step();
 (c) 8 x 2^22 samples, no burst, against corr_step_batched on the same input:
     what the candidate map and the lost early exit cost;
 (d) the row of (b) with 1024 bursts: the resolve pass's serial cost.

Results are merged into the output file shape by shape, so each shape can run
as a process of its own under its own time limit.

Usage: python scripts/corr_all_time.py [--out profiles/corr_all_time.json] [--shapes abcd]
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
    "a": dict(name="64ch x 16384, 4 bursts each", n=1 << 14, C=64, bursts=4, alts=("all", "bank_loop", "step_loop")),
    "b": dict(name="1 x 2^22, 64 bursts", n=1 << 22, C=1, bursts=64, alts=("all", "step_loop")),
    "c": dict(name="8ch x 2^22, no burst", n=1 << 22, C=8, bursts=0, alts=("all", "bank_step")),
    "d": dict(name="1 x 2^22, 1024 bursts", n=1 << 22, C=1, bursts=1024, alts=("all", "step_loop")),
}


def measure(key, shape, warmup, steps):
    C, n, B = shape["C"], shape["n"], shape["bursts"]
    g = torch.Generator(device="cuda").manual_seed(ord(key))
    x = torch.randint(-125, 126, (C, n, 2), dtype=torch.int16, device="cuda", generator=g)
    pats = [qpsk_pattern(N, 500, seed=c + 1) for c in range(C)]
    for c in range(C):
        p2 = torch.from_numpy((2 * pats[c]).astype(np.int16)).cuda()
        for k in range(B):
            off = ((2 * k + 1) * n) // (2 * B) - N
            x[c, off:off + N] += p2
    primed = []
    halo = torch.randint(-125, 126, (4096, 2), dtype=torch.int16, device="cuda", generator=g)
    for c in range(C):
        h = S.FixedPatternCorrelator(N, 1)
        h.setPattern(pats[c])
        h.prime(halo)
        primed.append(h)
    mh = max(2 * B, 4)

    def clones():
        return [copy.copy(h) for h in primed]

    def run_all(hs):  # the new call
        return [r[0].tolist() for r in S.corr_step_all_batched(hs, x, mh)]

    def step_loop(hs):  # the application's loop of step() on the remainders
        out = []
        for c in range(C):
            off, idx = 0, []
            while off < n:
                f, ci = hs[c].step(x[c, off:])
                if not f:
                    break
                idx.append(off + ci)
                off += ci + 2
            out.append(idx)
        return out

    def bank_loop(hs):  # corr_step_batched on the channels' common remaining prefix, round after round
        pos, out = [0] * C, [[] for _ in range(C)]
        while True:
            act = [c for c in range(C) if pos[c] < n]
            if not act:
                return out
            m = min(n - pos[c] for c in act)
            rows = torch.stack([x[c, pos[c]:pos[c] + m] for c in act])
            for (f, ci), c in zip(S.corr_step_batched([hs[c] for c in act], rows), act):
                if f:
                    out[c].append(pos[c] + ci)
                pos[c] += ci + 2 if f else m

    def bank_step(hs):  # one first-detection call (shape c: nothing to find)
        return [[ci] if f else [] for f, ci in S.corr_step_batched(hs, x)]

    fns = {"all": run_all, "step_loop": step_loop, "bank_loop": bank_loop, "bank_step": bank_step}
    alts = shape["alts"]
    # the same stream from the same state through every alternative
    k0, l0 = S.corr_all_stats()
    sets = {a: clones() for a in alts}
    res = {a: fns[a](sets[a]) for a in alts}
    k1, l1 = S.corr_all_stats()
    for a in alts[1:]:
        if res[a] != res["all"]:
            raise SystemExit(f"shape {key}: {a} and the new call disagree on the detections")
        if a != "bank_loop":  # its calls end elsewhere, so the registers differ in time, not in value
            for c in range(C):
                if (sets[a][c].getStatus() != sets["all"][c].getStatus() or
                        not np.array_equal(sets[a][c].getRefBitSamples(), sets["all"][c].getRefBitSamples())):
                    raise SystemExit(f"shape {key}: {a} and the new call leave channel {c} differently")
    hits = sum(len(r) for r in res["all"])
    if hits != C * B:
        raise SystemExit(f"shape {key}: {hits} detections, not the {C * B} the signal was built for")
    names = [a + s for s in ("", "_again") for a in alts]
    t = {k: [] for k in names}
    for i in range(warmup + steps):
        hs = [clones() for _ in names]
        for k, h in zip(names, hs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[k.replace("_again", "")](h)
            torch.cuda.synchronize()
            if i >= warmup:
                t[k].append(time.perf_counter() - t0)
    ms = {k: 1e3 * float(np.mean(v)) for k, v in t.items()}
    r = {
        "shape": shape["name"], "channels": C, "samples_per_channel": n, "N": N, "S": 1, "detections": hits,
        "path": "kernels" if (k1 - k0, l1 - l0) == (1, 0) else "loop", "warmup": warmup, "steps": steps,
        "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
        "spread_ms": {a: round(abs(ms[a] - ms[a + "_again"]), 5) for a in alts},
        "all_over": {a: round(min(ms["all"], ms["all_again"]) / min(ms[a], ms[a + "_again"]), 4) for a in alts[1:]},
    }
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_all_time.json"))
    ap.add_argument("--shapes", default="abcd")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corr_all_time.py needs a GPU")
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0),
                "protocol": "wall clock per call between device synchronisations, fresh clones of primed handles "
                            "per round; the alternatives alternate, each twice per round; means"})
    res.setdefault("results", {})
    for k in a.shapes:
        res["results"][k] = measure(k, SHAPES[k], a.warmup, a.steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
