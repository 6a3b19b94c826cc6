"""Time the DDC bank (srcdsp_mixdecim_step_batched) against the loop of
srcdsp_mixdecim_step over the same handles.  One process, device-resident data,
HIP events on the launch stream, 100 warm-up steps, mean of 200 timed steps; the
batched call and the loop alternate, and the loop is timed twice per round so
its own run-to-run spread is on record.  Needs a GPU (no fallback).

Shapes: (a) one shared input of 2^26 samples, C = 8, 127 taps; (b) the same
with 31 taps; (c) C = 64 independent inputs of 65 536 samples, 127 taps.  M = 4,
mixer N = 4096, Q14 Hamming-sinc taps.

Usage: python scripts/ddc_bank_time.py [--out profiles/ddc_bank_time.json] [--shapes abc]
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
SHAPES = {
    "a": dict(name="shared 2^26 x 8ch, 127 taps", shared=True, n=1 << 26, C=8, ntaps=127),
    "b": dict(name="shared 2^26 x 8ch, 31 taps", shared=True, n=1 << 26, C=8, ntaps=31),
    "c": dict(name="independent 64ch x 65536, 127 taps", shared=False, n=65536, C=64, ntaps=127),
}
CI16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")


def bank(C, cq):
    ms, ds = [], []
    for c in range(C):
        m = S.Mixer(4096)
        m.reset(FREQS[c % len(FREQS)] + 0.001 * (c // len(FREQS)))
        ms.append(m)
        ds.append(S.FilterDnsamplingFir(cq, 4, *CI16))
    return ms, ds


def measure(key, shape, warmup, steps):
    C, n, shared = shape["C"], shape["n"], shape["shared"]
    cq = q14(hamming_sinc(shape["ntaps"]))
    x = torch.randint(-32768, 32768, ((n, 2) if shared else (C, n, 2)), dtype=torch.int16, device="cuda")
    y = torch.empty((C, n // 4, 2), dtype=torch.int16, device="cuda")
    y2 = torch.empty_like(y)
    ms, ds = bank(C, cq)
    chains = [S.MixerDecimatorChain(m, d) for m, d in zip(ms, ds)]
    rows = [x if shared else x[c] for c in range(C)]

    def batched():
        S.mixdecim_step_batched(ms, ds, x, y)

    def loop():
        for c in range(C):
            chains[c].step(rows[c], y2[c])

    # the same step from the same state through both paths: identical outputs
    mc, dc = [copy.copy(m) for m in ms], [copy.copy(d) for d in ds]
    b0, l0 = S.mixdecim_batched_stats()
    batched()
    b1, l1 = S.mixdecim_batched_stats()
    for c in range(C):
        S.MixerDecimatorChain(mc[c], dc[c]).step(rows[c], y2[c])
    torch.cuda.synchronize()
    if not torch.equal(y, y2):
        raise SystemExit(f"shape {key}: the batched call and the loop disagree")
    path = "bank kernel" if b1 - b0 == 1 else "per-channel loop"

    st = torch.cuda.current_stream()
    for _ in range(warmup):
        batched()
        loop()
    names = ("batched", "loop", "loop_again")
    fns = (batched, loop, loop)
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
    # per input sample: the bank kernel reads a shared input once (4 B) and writes C outputs of 4 B per 4 samples
    bytes_loop = 5 * C
    bytes_batched = (4 + C) if shared and path == "bank kernel" else bytes_loop
    r = {
        "shape": shape["name"], "channels": C, "samples_per_channel": n, "ntaps": shape["ntaps"], "M": 4, "N": 4096,
        "batched_path": path,
        "ms_per_step": {k: round(v, 5) for k, v in ms_.items()},
        "loop_spread_ms": round(abs(ms_["loop"] - ms_["loop_again"]), 5),
        "bytes_per_input_sample": {"batched": bytes_batched, "loop": bytes_loop},
        "GB_per_s": {"batched": round(bytes_batched * n / ms_["batched"] / 1e6, 1),
                     "loop": round(bytes_loop * n / ms_["loop"] / 1e6, 1)},
        "batched_over_loop": round(ms_["batched"] / min(ms_["loop"], ms_["loop_again"]), 4),
    }
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddc_bank_time.json"))
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ddc_bank_time.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; batched, loop, loop alternate per step; means",
           "results": {k: measure(k, SHAPES[k], a.warmup, a.steps) for k in a.shapes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
