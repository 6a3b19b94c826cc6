"""Time the interpolator -> mixer chain (srcdsp_upmix_step, srcdsp_upmix_step_batched)
against the pair of calls srcdsp_up_step; srcdsp_mixer_step on the same
handles.  One process, device-resident data, HIP events on the launch stream,
100 warm-up steps, mean of 200 timed steps; the fused call and the pair
alternate, and the pair is timed twice per round so its own run-to-run spread
is on record (a shape counts as a win only when the fused time is below the
faster pair timing by more than that spread).  The single-channel shapes also
time the interpolator alone.  Needs a GPU (no fallback).

Shapes: (a) L = 4, 128 taps, 2^26 inputs, one channel (the `up` bench shape);
(b) the same with 64 taps; (c) 64 channels of 65 536 inputs, 128 taps: the
batched call against the loop of 64 pairs.  Mixer N = 4096, Q14 Hamming-sinc taps.

Usage: python scripts/upmix_time.py [--out profiles/upmix_time.json] [--shapes abc]
       [--warmup 100] [--steps 200]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import srcdsp_amd as S
from srcdsp_amd.design import hamming_sinc, q14

FREQS = [0.0, 0.1, -0.37, 0.5, 0.73, -0.2, 0.3, -0.45]
L = 4
SHAPES = {
    "a": dict(name="1ch x 2^26, L=4, 128 taps", n=1 << 26, C=1, ntaps=128),
    "b": dict(name="1ch x 2^26, L=4, 64 taps", n=1 << 26, C=1, ntaps=64),
    "c": dict(name="64ch x 65536, L=4, 128 taps", n=65536, C=64, ntaps=128),
}


def bank(C, cq):
    ups, ms = [], []
    for c in range(C):
        ups.append(S.FilterUpsamplingFir(cq, L))
        m = S.Mixer(4096)
        m.reset(FREQS[c % len(FREQS)] + 0.001 * (c // len(FREQS)))
        ms.append(m)
    return ups, ms


def measure(key, shape, warmup, steps):
    C, n = shape["C"], shape["n"]
    cq = q14(hamming_sinc(shape["ntaps"], 0.48 / L) * L)
    x = torch.randint(-32768, 32768, (C, n, 2), dtype=torch.int16, device="cuda")
    y = torch.empty((C, L * n, 2), dtype=torch.int16, device="cuda")
    tmp = torch.empty_like(y)
    y2 = torch.empty_like(y)
    ups, ms = bank(C, cq)
    chain0 = S.UpsamplerMixerChain(ups[0], ms[0])

    def fused():
        if C == 1:
            chain0.step(x[0], y[0])
        else:
            S.upmix_step_batched(ups, ms, x, y)

    def pair():
        for c in range(C):
            ms[c].step(ups[c].step(x[c], tmp[c]), y2[c])

    def up_only():
        ups[0].step(x[0], tmp[0])

    # the same step from the same state through both paths: identical outputs
    uc, mc = [copy.copy(u) for u in ups], [copy.copy(m) for m in ms]
    s0 = S.upmix_stats()
    fused()
    s1 = S.upmix_stats()
    for c in range(C):
        mc[c].step(uc[c].step(x[c], tmp[c]), y2[c])
    torch.cuda.synchronize()
    if not torch.equal(y, y2):
        raise SystemExit(f"shape {key}: the fused call and the pair of calls disagree")
    path = ("fused kernel", "pair inside the call", "bank launch", "per-channel loop")[
        [b - a for a, b in zip(s0, s1)].index(1)]

    st = torch.cuda.current_stream()
    for _ in range(warmup):
        fused()
        pair()
    names = ("fused", "pair", "pair_again") + (("up_only",) if C == 1 else ())
    fns = (fused, pair, pair) + ((up_only,) if C == 1 else ())
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k in names}
    for i in range(steps):
        for k, fn in zip(names, fns):
            a, b = ev[k][i]
            a.record(st)
            fn()
            b.record(st)
    torch.cuda.synchronize()
    ms_ = {k: float(np.mean([a.elapsed_time(b) for a, b in ev[k]])) for k in names}
    spread = abs(ms_["pair"] - ms_["pair_again"])
    best_pair = min(ms_["pair"], ms_["pair_again"])
    # per input sample and channel: 4 B read, 4 L B written; the pair writes, reads and writes the L outputs
    bytes_fused, bytes_pair = 4 + 4 * L, 4 + 3 * 4 * L
    r = {
        "shape": shape["name"], "channels": C, "inputs_per_channel": n, "ntaps": shape["ntaps"], "L": L, "N": 4096,
        "fused_path": path,
        "ms_per_step": {k: round(v, 5) for k, v in ms_.items()},
        "pair_spread_ms": round(spread, 5),
        "bytes_per_input_sample": {"fused": bytes_fused, "pair": bytes_pair},
        "GB_per_s": {"fused": round(bytes_fused * C * n / ms_["fused"] / 1e6, 1),
                     "pair": round(bytes_pair * C * n / best_pair / 1e6, 1)},
        "fused_over_pair": round(ms_["fused"] / best_pair, 4),
        "fused_wins": bool(ms_["fused"] < best_pair - spread),
    }
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upmix_time.json"))
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upmix_time.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; fused, pair, pair (, interpolator alone) alternate per step; means",
           "results": {k: measure(k, SHAPES[k], a.warmup, a.steps) for k in a.shapes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
