"""Time the carrier combiner (srcdsp_combine_step), alone and behind the offset
modulator bank.  The protocol of scripts/oqpsk_time.py: one process,
device-resident data, HIP events on the launch stream, 100 warm-up steps, mean
of 200 timed steps; the alternatives alternate within every step and each is
timed twice per round, so its own run-to-run spread is on record.  Needs a GPU
(no fallback).

The combiner alone: 8 rows x 2^26 samples and 2 rows x 2^28 samples, against
(rows + 1) * 4 bytes per sample of the 8 TB/s HBM specification, with FilterFir
(float -> complex<float>, 31 taps, 12 bytes per sample) beside it in the same
process.

C carriers onto one wire, at D = L / 2 and N = 4096, QPSK and SDPSK each:
  (a) 8 carriers x 2^23 symbols, L = 4, 128 taps
  (b) 4 carriers x 2^24 symbols, L = 8, 64 taps
  (c) 64 carriers x 65 536 symbols, L = 4, 128 taps
  (d) 2 carriers x 2^25 symbols, L = 4, 64 taps
Alternatives: `bank_then_combine`, srcdsp_modulate_offset_step_batched into C
rows, then the combiner; `torch_sum`, what an application without the combiner
does on the device: the bank, then an int32 sum, shift and clamp in torch;
`bank`, the bank alone, so the combiner's share of the step is on record.  The
two composites are identical, checked before timing.

Usage: python scripts/carrier_sum_time.py [--out profiles/carrier_sum_time.json] [--shapes abcd]
       [--warmup 100] [--steps 200] [--no-combiner]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import srcdsp_amd as S
from srcdsp_amd.design import hamming_sinc, q14

HBM_SPEC = 8e12
KINDS = {"qpsk": (S.SymbolMapperQpsk, 2), "sdpsk": (S.SymbolMapperSdpsk, 1)}  # class, bits per symbol
SHAPES = {
    "a": dict(name="8 carriers x 2^23 symbols, L=4, 128 taps", n=1 << 23, C=8, L=4, ntaps=128),
    "b": dict(name="4 carriers x 2^24 symbols, L=8, 64 taps", n=1 << 24, C=4, L=8, ntaps=64),
    "c": dict(name="64 carriers x 65536 symbols, L=4, 128 taps", n=65536, C=64, L=4, ntaps=128),
    "d": dict(name="2 carriers x 2^25 symbols, L=4, 64 taps", n=1 << 25, C=2, L=4, ntaps=64),
}
SHIFT = 2


def timed(fns, warmup, steps):
    """fns: {name: callable}.  Mean ms per call of each, the callables
    alternating within every step."""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k in fns}
    for i in range(steps):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record(st)
            fn()
            b.record(st)
    torch.cuda.synchronize()
    return {k: float(np.mean([a.elapsed_time(b) for a, b in ev[k]])) for k in fns}


def twice(ms, k):
    """(the faster of an alternative's two timings, their difference)."""
    return min(ms[k], ms[k + "_again"]), abs(ms[k] - ms[k + "_again"])


def measure_combiner(rows, lg, warmup, steps):
    n = 1 << lg
    x = torch.empty((rows, n, 2), dtype=torch.int16, device="cuda")
    S.fill_synthetic(x, "ci16", lo=-32767, hi=32767)
    y = torch.empty((n, 2), dtype=torch.int16, device="cuda")
    xf = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    yf = torch.empty(n, dtype=torch.complex64, device="cuda")
    fir = S.FilterFir(hamming_sinc(31, 0.2), "float", "complex<float>", "float", "float")
    S.combine(x, y, SHIFT)
    k = 1 << 20  # a spot check of the first 2^20 samples against torch
    want = (x[:, :k].to(torch.int32).sum(0) >> SHIFT).clamp(-32768, 32767).to(torch.int16)
    if not torch.equal(y[:k], want):
        raise SystemExit("the combiner and torch disagree")
    ms = timed({"combine": lambda: S.combine(x, y, SHIFT), "fir": lambda: fir.step(xf, yf),
                "combine_again": lambda: S.combine(x, y, SHIFT), "fir_again": lambda: fir.step(xf, yf)}, warmup, steps)
    best, spread = twice(ms, "combine")
    fbest, fspread = twice(ms, "fir")
    bps = 4 * (rows + 1)
    r = {"rows": rows, "samples": n, "shift": SHIFT, "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
         "combine": {"bytes_per_sample": bps, "spread_ms": round(spread, 5),
                     "TB_per_s": round(bps * n / (1e-3 * best) / 1e12, 4),
                     "share_of_8TBps": round(bps * n / (1e-3 * best) / HBM_SPEC, 4)},
         "fir": {"bytes_per_sample": 12, "spread_ms": round(fspread, 5),
                 "TB_per_s": round(12 * n / (1e-3 * fbest) / 1e12, 4),
                 "share_of_8TBps": round(12 * n / (1e-3 * fbest) / HBM_SPEC, 4)}}
    print(json.dumps(r), flush=True)
    return r


def measure_sum(key, kind, shape, warmup, steps):
    cls, bps = KINDS[kind]
    C, n, L = shape["C"], shape["n"], shape["L"]
    D = L // 2
    cq = q14(hamming_sinc(shape["ntaps"], 0.48 / L) * L / C)  # C carriers share the wire's range
    bits = torch.randint(0, 2, (C, bps * n), dtype=torch.uint8, device="cuda")
    rows = torch.empty((C, L * n, 2), dtype=torch.int16, device="cuda")
    wire = torch.empty((L * n, 2), dtype=torch.int16, device="cuda")
    wire2 = torch.empty_like(wire)
    hs = [[], [], [], []]
    for c in range(C):
        m = S.Mixer(4096)
        m.reset(-0.9 + 1.8 * (c + 0.5) / C)
        for lst, h in zip(hs, (cls(), S.FilterUpsamplingFir(cq, L), S.QStagger(D), m)):
            lst.append(h)

    def bank(h=hs):
        S.modulate_offset_step_batched(*h, bits, rows)

    def bank_then_combine(h=hs, out=wire):
        S.modulate_offset_step_batched(*h, bits, rows)
        S.combine(rows, out, SHIFT)

    def torch_sum(h=hs):
        S.modulate_offset_step_batched(*h, bits, rows)
        (rows.to(torch.int32).sum(0) >> SHIFT).clamp(-32768, 32767).to(torch.int16)

    b0 = S.modulate_offset_stats()
    bank_then_combine()
    b1 = S.modulate_offset_stats()
    wire2.copy_((rows.to(torch.int32).sum(0) >> SHIFT).clamp(-32768, 32767))
    torch.cuda.synchronize()
    if not torch.equal(wire, wire2):
        raise SystemExit(f"shape {key} {kind}: the combiner and torch disagree")
    peak = int(wire.abs().max())
    inner = ("fused kernel", "four operators", "bank launch", "per-channel loop")[[b - a for a, b in zip(b0, b1)].index(1)]
    fns = {"bank": bank, "bank_then_combine": bank_then_combine, "torch_sum": torch_sum}
    fns.update({k + "_again": v for k, v in list(fns.items())})
    ms = timed(fns, warmup, steps)
    bnk, bnk_spread = twice(ms, "bank")
    seq, seq_spread = twice(ms, "bank_then_combine")
    tor, tor_spread = twice(ms, "torch_sum")
    # per symbol: the bank reads the bits and writes C * 4 L bytes; the combiner reads them and writes 4 L
    moved = C * (bps + (1.5 if kind == "sdpsk" else 0)) + (2 * C + 1) * 4 * L
    r = {"shape": f"{shape['name']}, D={D}", "kind": kind, "channels": C, "symbols_per_channel": n, "L": L, "D": D,
         "ntaps": shape["ntaps"], "N": 4096, "shift": SHIFT, "bank_path": inner, "peak_of_composite": peak,
         "ms_per_step": {k: round(v, 5) for k, v in ms.items()},
         "spread_ms": {"bank": round(bnk_spread, 5), "bank_then_combine": round(seq_spread, 5),
                       "torch_sum": round(tor_spread, 5)},
         "combiner_ms": round(seq - bnk, 5), "torch_sum_ms": round(tor - bnk, 5),
         "bytes_per_symbol": moved, "GB_per_s": round(moved * n / seq / 1e6, 1),
         "bank_then_combine_over_torch_sum": round(seq / tor, 4)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carrier_sum_time.json"))
    ap.add_argument("--shapes", default="abcd")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--no-combiner", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carrier_sum_time.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; the alternatives alternate per step, each timed twice; means",
           "combiner": {}, "one_wire": {}}
    if not a.no_combiner:
        for rows, lg in ((8, 26), (2, 28)):
            res["combiner"][f"{rows}x2^{lg}"] = measure_combiner(rows, lg, a.warmup, a.steps)
            torch.cuda.empty_cache()
    for k in a.shapes:
        for kind in KINDS:
            res["one_wire"][f"{k}_{kind}"] = measure_sum(k, kind, SHAPES[k], a.warmup, a.steps)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
