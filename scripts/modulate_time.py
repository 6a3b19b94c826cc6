"""Time the transmit chain from bits (srcdsp_modulate_step, srcdsp_modulate_step_batched)
against the sequence srcdsp_mapper_step; srcdsp_upmix_step on the same
handles, and the mappers alone.  The protocol of scripts/upmix_time.py: one
process, device-resident data, HIP events on the launch stream, 100 warm-up
steps, mean of 200 timed steps; the fused call and the sequence alternate, and
the sequence is timed twice per round so its own run-to-run spread is on
record (a shape counts as a win only when the fused time is below the faster
sequence timing by more than that spread).  Needs a GPU (no fallback).

Shapes, for both mapper kinds, L = 4, mixer N = 4096, Q14 Hamming-sinc taps:
(a) 2^26 symbols, 128 taps; (b) 2^26 symbols, 64 taps; (c) 64 rows x 65 536
symbols, 128 taps: the batched call against the loop of 64 sequences.
(m) srcdsp_mapper_step alone at 2^28 bits, bytes moved over time against the
8 TB/s HBM specification, with srcdsp_freqest_run over 2^28 samples beside it
in the same process as the box's streaming yardstick.  (k) the mapper bank at
64 x 4096 and 1024 x 4096 bits against the loop of single calls.

Usage: python scripts/modulate_time.py [--out profiles/modulate_time.json] [--shapes abcmk]
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
HBM_SPEC_TBS = 8.0
KINDS = {"sdpsk": (S.SymbolMapperSdpsk, 1), "qpsk": (S.SymbolMapperQpsk, 2)}  # class, bits per symbol
SHAPES = {
    "a": dict(name="1ch x 2^26 symbols, L=4, 128 taps", n=1 << 26, C=1, ntaps=128),
    "b": dict(name="1ch x 2^26 symbols, L=4, 64 taps", n=1 << 26, C=1, ntaps=64),
    "c": dict(name="64ch x 65536 symbols, L=4, 128 taps", n=65536, C=64, ntaps=128),
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


def bits_tensor(shape):
    return torch.randint(0, 2, shape, dtype=torch.uint8, device="cuda")


def measure_chain(key, kind, shape, warmup, steps):
    cls, bps = KINDS[kind]
    C, n = shape["C"], shape["n"]
    cq = q14(hamming_sinc(shape["ntaps"], 0.48 / L) * L)
    bits = bits_tensor((C, bps * n))
    y = torch.empty((C, L * n, 2), dtype=torch.int16, device="cuda")
    y2 = torch.empty_like(y)
    sym = torch.empty((C, n, 2), dtype=torch.int16, device="cuda")
    maps, ups, ms = [], [], []
    for c in range(C):
        maps.append(cls())
        ups.append(S.FilterUpsamplingFir(cq, L))
        m = S.Mixer(4096)
        m.reset(FREQS[c % len(FREQS)] + 0.001 * (c // len(FREQS)))
        ms.append(m)
    chain0 = S.ModulatorChain(maps[0], ups[0], ms[0])
    seqs = [S.UpsamplerMixerChain(ups[c], ms[c]) for c in range(C)]

    def fused():
        if C == 1:
            chain0.step(bits[0], y[0])
        else:
            S.modulate_step_batched(maps, ups, ms, bits, y)

    def sequence(mp=maps, sq=seqs):
        for c in range(C):
            sq[c].step(mp[c].step(bits[c], sym[c]), y2[c])

    # the same step from the same state through both paths: identical outputs
    mc, uc, xc = [copy.copy(v) for v in maps], [copy.copy(v) for v in ups], [copy.copy(v) for v in ms]
    s0 = S.modulate_stats()
    fused()
    s1 = S.modulate_stats()
    sequence(mc, [S.UpsamplerMixerChain(uc[c], xc[c]) for c in range(C)])
    torch.cuda.synchronize()
    if not torch.equal(y, y2):
        raise SystemExit(f"shape {key} {kind}: the fused call and the sequence disagree")
    path = ("fused kernel", "sequence inside the call", "bank launch", "per-channel loop")[
        [b - a for a, b in zip(s0, s1)].index(1)]

    ms_ = timed(("fused", "sequence", "sequence_again"), (fused, sequence, sequence), warmup, steps)
    spread = abs(ms_["sequence"] - ms_["sequence_again"])
    best = min(ms_["sequence"], ms_["sequence_again"])
    # per symbol and channel: the fused call reads the bits (SDPSK: twice, and writes and reads 1/4 byte of
    # states) and writes 4 L bytes; the sequence also writes and reads the 4-byte symbol
    extra = 1.5 if kind == "sdpsk" else 0
    bytes_fused, bytes_seq = bps + extra + 4 * L, bps + (1 if kind == "sdpsk" else 0) + 8 + 4 * L
    r = {
        "shape": shape["name"], "kind": kind, "channels": C, "symbols_per_channel": n, "ntaps": shape["ntaps"], "L": L,
        "N": 4096, "fused_path": path,
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


def measure_mapper_stream(warmup, steps):
    n = 1 << 28
    out = {}
    bits = bits_tensor((n,))
    for kind, (cls, bps) in KINDS.items():
        y = torch.empty((n // bps, 2), dtype=torch.int16, device="cuda")
        m = cls()
        t = timed(("mapper",), (lambda: m.step(bits, y),), warmup, steps)["mapper"]
        moved = n * ((2 if kind == "sdpsk" else 1) + 4 / bps)  # SDPSK reads the bits twice
        out[kind] = {"bits": n, "ms_per_step": round(t, 5), "bytes_moved": int(moved),
                     "TB_per_s": round(moved / t / 1e9, 3), "of_hbm_spec": round(moved / t / 1e9 / HBM_SPEC_TBS, 3)}
        print(json.dumps({kind: out[kind]}), flush=True)
        del y
    del bits
    x = torch.randint(-2048, 2048, (n, 2), dtype=torch.int16, device="cuda")
    fe = S.FreqEstimator(1)
    t = timed(("freqest",), (lambda: fe.run(x),), max(warmup // 4, 5), max(steps // 4, 10))["freqest"]
    out["freqest_yardstick"] = {"samples": n, "ms_per_step": round(t, 5), "bytes_moved": 4 * n,
                                "TB_per_s": round(4 * n / t / 1e9, 3)}
    print(json.dumps({"freqest_yardstick": out["freqest_yardstick"]}), flush=True)
    return out


def measure_mapper_bank(warmup, steps):
    out = {}
    for rows in (64, 1024):
        for kind, (cls, bps) in KINDS.items():
            n = 4096
            bits = bits_tensor((rows, n))
            y = torch.empty((rows, n // bps, 2), dtype=torch.int16, device="cuda")
            y2 = torch.empty_like(y)
            maps = [cls() for _ in range(rows)]

            def bank():
                S.mapper_step_batched(maps, bits, y)

            def loop():
                for c in range(rows):
                    maps[c].step(bits[c], y2[c])

            t = timed(("bank", "loop", "loop_again"), (bank, loop, loop), warmup, steps)
            if not torch.equal(y, y2):
                raise SystemExit(f"mapper bank {rows} x {n} {kind}: the bank and the loop disagree")
            best = min(t["loop"], t["loop_again"])
            out[f"{rows}x{n}_{kind}"] = {"rows": rows, "bits_per_row": n, "kind": kind,
                                         "ms_per_step": {k: round(v, 5) for k, v in t.items()},
                                         "loop_spread_ms": round(abs(t["loop"] - t["loop_again"]), 5),
                                         "loop_over_bank": round(best / t["bank"], 2)}
            print(json.dumps(out[f"{rows}x{n}_{kind}"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modulate_time.json"))
    ap.add_argument("--shapes", default="abcmk")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("modulate_time.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; fused, sequence, sequence alternate per step; means",
           "results": {}}
    for k in a.shapes:
        if k in SHAPES:
            for kind in KINDS:
                res["results"][f"{k}_{kind}"] = measure_chain(k, kind, SHAPES[k], a.warmup, a.steps)
        elif k == "m":
            res["mapper_stream"] = measure_mapper_stream(a.warmup, a.steps)
        elif k == "k":
            res["mapper_bank"] = measure_mapper_bank(a.warmup, a.steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
