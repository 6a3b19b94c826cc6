"""Time the offset-QPSK transmit chain from bits (srcdsp_modulate_offset_step,
srcdsp_modulate_offset_step_batched) against the four-call sequence
srcdsp_mapper_step; srcdsp_up_step; srcdsp_stagger_step; srcdsp_mixer_step (in
place) on the same handles.  The protocol of scripts/modulate_time.py: one
process, device-resident data, HIP events on the launch stream, 100 warm-up
steps, mean of 200 timed steps; the fused call and the sequence alternate, and
the sequence is timed twice per round so its own run-to-run spread is on
record (a shape counts as a win only when the fused time is below the faster
sequence timing by more than that spread).  Needs a GPU (no fallback).

Shapes, for both mapper kinds, L = 4 and L = 8, D = L / 2, mixer N = 4096, Q14
Hamming-sinc taps: (a) 2^26 symbols, 128 taps; (b) 2^26 symbols, 64 taps;
(c) 64 rows x 65 536 symbols, 128 taps: the batched call against the loop of
64 sequences.

Usage: python scripts/oqpsk_time.py [--out profiles/oqpsk_time.json] [--shapes abc] [--L 4,8]
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
KINDS = {"sdpsk": (S.SymbolMapperSdpsk, 1), "qpsk": (S.SymbolMapperQpsk, 2)}  # class, bits per symbol
SHAPES = {
    "a": dict(name="1ch x 2^26 symbols, 128 taps", n=1 << 26, C=1, ntaps=128),
    "b": dict(name="1ch x 2^26 symbols, 64 taps", n=1 << 26, C=1, ntaps=64),
    "c": dict(name="64ch x 65536 symbols, 128 taps", n=65536, C=64, ntaps=128),
}


def timed(names, fns, warmup, steps):
    """Mean ms per call of each fn, the fns alternating within every step."""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k in names}
    for i in range(steps):
        for k, fn in zip(names, fns):
            a, b = ev[k][i]
            a.record(st)
            fn()
            b.record(st)
    torch.cuda.synchronize()
    return {k: float(np.mean([a.elapsed_time(b) for a, b in ev[k]])) for k in names}


def measure_chain(key, kind, L, shape, warmup, steps):
    cls, bps = KINDS[kind]
    C, n, D = shape["C"], shape["n"], L // 2
    cq = q14(hamming_sinc(shape["ntaps"], 0.48 / L) * L)
    bits = torch.randint(0, 2, (C, bps * n), dtype=torch.uint8, device="cuda")
    y = torch.empty((C, L * n, 2), dtype=torch.int16, device="cuda")
    y2 = torch.empty_like(y)
    sym = torch.empty((C, n, 2), dtype=torch.int16, device="cuda")
    tmp = torch.empty((L * n, 2), dtype=torch.int16, device="cuda")  # the interpolator's output, one row at a time
    maps, ups, gs, ms = [], [], [], []
    for c in range(C):
        maps.append(cls())
        ups.append(S.FilterUpsamplingFir(cq, L))
        gs.append(S.QStagger(D))
        m = S.Mixer(4096)
        m.reset(FREQS[c % len(FREQS)] + 0.001 * (c // len(FREQS)))
        ms.append(m)
    chain0 = S.OffsetModulatorChain(maps[0], ups[0], gs[0], ms[0])

    def fused():
        if C == 1:
            chain0.step(bits[0], y[0])
        else:
            S.modulate_offset_step_batched(maps, ups, gs, ms, bits, y)

    def sequence(mp=maps, up=ups, sg=gs, mx=ms):
        for c in range(C):
            up[c].step(mp[c].step(bits[c], sym[c]), tmp)
            mx[c].step(sg[c].step(tmp, y2[c]), y2[c])  # the mixer in place: it is element-wise

    # the same step from the same state through both paths: identical outputs
    clones = [[copy.copy(v) for v in hs] for hs in (maps, ups, gs, ms)]
    s0 = S.modulate_offset_stats()
    fused()
    s1 = S.modulate_offset_stats()
    sequence(*clones)
    torch.cuda.synchronize()
    if not torch.equal(y, y2):
        raise SystemExit(f"shape {key} {kind} L={L}: the fused call and the sequence disagree")
    path = ("fused kernel", "sequence inside the call", "bank launch", "per-channel loop")[
        [b - a for a, b in zip(s0, s1)].index(1)]

    ms_ = timed(("fused", "sequence", "sequence_again"), (fused, sequence, sequence), warmup, steps)
    spread = abs(ms_["sequence"] - ms_["sequence_again"])
    best = min(ms_["sequence"], ms_["sequence_again"])
    # per symbol and channel: the fused call reads the bits (SDPSK: twice, and writes and reads 1/4 byte of
    # states) and writes 4 L bytes; the sequence also writes and reads the 4-byte symbol, writes and reads the
    # interpolator's 4 L bytes, and reads and rewrites the 4 L bytes the mixer works on in place
    extra = 1.5 if kind == "sdpsk" else 0
    bytes_fused = bps + extra + 4 * L
    bytes_seq = bps + (1 if kind == "sdpsk" else 0) + 8 + 4 * 4 * L
    r = {
        "shape": f"{shape['name']}, L={L}, D={D}", "kind": kind, "channels": C, "symbols_per_channel": n,
        "ntaps": shape["ntaps"], "L": L, "D": D, "N": 4096, "fused_path": path,
        "ms_per_step": {k: round(v, 5) for k, v in ms_.items()},
        "sequence_spread_ms": round(spread, 5),
        "bytes_per_symbol": {"fused": bytes_fused, "sequence": bytes_seq},
        "GB_per_s": {"fused": round(bytes_fused * C * n / ms_["fused"] / 1e6, 1),
                     "sequence": round(bytes_seq * C * n / best / 1e6, 1)},
        "fused_over_sequence": round(ms_["fused"] / best, 4),
        "fused_wins": bool(ms_["fused"] < best - spread),
        "fused_loses": bool(ms_["fused"] > best + spread),
    }
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oqpsk_time.json"))
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--L", default="4,8")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("oqpsk_time.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; fused, sequence, sequence alternate per step; means",
           "results": {}}
    for k in a.shapes:
        for L in (int(v) for v in a.L.split(",")):
            for kind in KINDS:
                res["results"][f"{k}_L{L}_{kind}"] = measure_chain(k, kind, L, SHAPES[k], a.warmup, a.steps)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
