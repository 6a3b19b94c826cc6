"""Time the interpolator -> decimator chain (srcdsp_resample_step,
srcdsp_resample_step_batched) with the fused kernel forced
(resample_set_min_tiles(1)) against the sequence srcdsp_up_step;
srcdsp_decim_step on the same handles.  The protocol of scripts/upmix_time.py:
one process, device-resident data, HIP events on the launch stream, 100 warm-up
steps, mean of 200 timed steps; the fused call and the sequence alternate, and
the sequence is timed twice per round so its own run-to-run spread is on record
(a shape counts as a win only when the fused time is below the faster sequence
timing by more than that spread).  Needs a GPU (no fallback).

Shapes (L / M, interpolator taps, decimator taps): (a) 4/3, 128, 96; (b) 2/3,
64, 63; (c) 8/5, 128, 100 on 2^25 inputs; (d) 4/4, 128, 127; (e) shape (a) as
64 rows of 65 536 inputs, the bank against the loop of 64 sequences.  (a), (b)
and (d) run on 2^26 inputs.  (f), (g): (a) and (b) on 2^22 inputs, (h): (b) as
the bank of (e) -- the shortest calls the routing sends to the kernel.  Input
lengths are rounded down to the next length with L n a multiple of M and n a
multiple of 4.  Q14 Hamming-sinc taps.

Usage: python scripts/resample_time.py [--out profiles/resample_time.json] [--shapes abcdefgh]
       [--warmup 100] [--steps 200]"""
import argparse
import copy
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import srcdsp_amd as S
from srcdsp_amd.design import hamming_sinc, q14

CI16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")
SHAPES = {
    "a": dict(L=4, M=3, nu=128, nd=96, n=1 << 26, C=1),
    "b": dict(L=2, M=3, nu=64, nd=63, n=1 << 26, C=1),
    "c": dict(L=8, M=5, nu=128, nd=100, n=1 << 25, C=1),
    "d": dict(L=4, M=4, nu=128, nd=127, n=1 << 26, C=1),
    "e": dict(L=4, M=3, nu=128, nd=96, n=65536, C=64),
    # the shortest calls the routing sends to the kernel: 2048 tiles, one row and 64 rows
    "f": dict(L=4, M=3, nu=128, nd=96, n=1 << 22, C=1),
    "g": dict(L=2, M=3, nu=64, nd=63, n=1 << 22, C=1),
    "h": dict(L=2, M=3, nu=64, nd=63, n=65536, C=64),
}


def whole(n, L, M):
    g = M // math.gcd(L, M)
    q = g * 4 // math.gcd(g, 4)
    return n // q * q


def measure(key, shape, warmup, steps):
    L, M, C = shape["L"], shape["M"], shape["C"]
    n = whole(shape["n"], L, M)
    n_out = L * n // M
    cu = q14(hamming_sinc(shape["nu"], 0.48 / L) * L)
    cd = q14(hamming_sinc(shape["nd"], 0.48 / max(L, M)))
    x = torch.randint(-32768, 32768, (C, n, 2), dtype=torch.int16, device="cuda")
    y = torch.empty((C, n_out, 2), dtype=torch.int16, device="cuda")
    y2 = torch.empty_like(y)
    tmp = torch.empty((C, L * n, 2), dtype=torch.int16, device="cuda")
    ups = [S.FilterUpsamplingFir(cu, L, *CI16) for _ in range(C)]
    decs = [S.FilterDnsamplingFir(cd, M, *CI16) for _ in range(C)]
    chain0 = S.RationalResampler(ups[0], decs[0])

    def fused():
        if C == 1:
            chain0.step(x[0], y[0])
        else:
            S.resample_step_batched(ups, decs, x, y)

    def pair():
        for c in range(C):
            decs[c].step(ups[c].step(x[c], tmp[c]), y2[c])

    # the same step from the same state through both paths: identical outputs
    uc, dc = [copy.copy(u) for u in ups], [copy.copy(d) for d in decs]
    s0 = S.resample_stats()
    fused()
    s1 = S.resample_stats()
    for c in range(C):
        dc[c].step(uc[c].step(x[c], tmp[c]), y2[c])
    torch.cuda.synchronize()
    if not torch.equal(y, y2):
        raise SystemExit(f"shape {key}: the fused call and the sequence of calls disagree")
    path = ("fused kernel", "pair inside the call", "bank launch", "per-channel loop")[
        [b - a for a, b in zip(s0, s1)].index(1)]

    st = torch.cuda.current_stream()
    for _ in range(warmup):
        fused()
        pair()
    names = ("fused", "pair", "pair_again")
    fns = (fused, pair, pair)
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
    # per input sample and channel: 4 B read, 4 L / M B written; the sequence also writes and reads the L mid words
    bytes_fused, bytes_pair = 4 + 4 * L / M, 4 + 8 * L + 4 * L / M
    r = {
        "shape": f"{C}ch x {n}, L/M = {L}/{M}, {shape['nu']} / {shape['nd']} taps", "channels": C,
        "inputs_per_channel": n, "L": L, "M": M, "up_taps": shape["nu"], "decim_taps": shape["nd"],
        "fused_path": path,
        "ms_per_step": {k: round(v, 5) for k, v in ms_.items()},
        "pair_spread_ms": round(spread, 5),
        "bytes_per_input_sample": {"fused": round(bytes_fused, 3), "pair": round(bytes_pair, 3)},
        "GB_per_s": {"fused": round(bytes_fused * C * n / ms_["fused"] / 1e6, 1),
                     "pair": round(bytes_pair * C * n / best_pair / 1e6, 1)},
        "fused_over_pair": round(ms_["fused"] / best_pair, 4),
        "fused_wins": bool(ms_["fused"] < best_pair - spread),
    }
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.json"))
    ap.add_argument("--shapes", default="abcdefgh")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py needs a GPU")
    S.resample_set_min_tiles(1)  # the fused kernel on every shape it takes, whatever the routing
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; fused (kernel forced), pair, pair alternate per step; means",
           "results": {}}
    for k in a.shapes:
        res["results"][k] = measure(k, SHAPES[k], a.warmup, a.steps)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
