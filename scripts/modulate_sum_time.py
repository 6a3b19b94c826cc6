"""Time the summing modulator bank (srcdsp_modulate_sum_step) against the pair
it replaces, srcdsp_modulate_offset_step_batched into C rows followed by
srcdsp_combine_step.  The protocol of scripts/carrier_sum_time.py: one process,
device-resident data, HIP events on the launch stream, 100 warm-up steps, mean
of 200 timed steps; the alternatives alternate within every step and each is
timed twice per round, so its own run-to-run spread is on record.  Needs a GPU
(no fallback).

`one_wire`: the shapes (a)-(d) of carrier_sum_time.py at D = L / 2 and
N = 4096, QPSK and SDPSK each.  Alternatives: `sum`, the new call with the
routing threshold at one tile, so the fused kernel serves it wherever it takes
the shape; `pair`, the bank into C rows, then the combiner; `bank`, the bank
alone, which bounds what fusing the sum can gain.  The two wires are
identical, checked before timing.

`threshold`: the same two alternatives over rows of 2^k tiles of 2048 symbols,
L in {2, 4, 8} and C in {2, 8, 64}, QPSK: the tile count from which the fused
kernel is faster than the pair by more than the pair's twice-timed spread, at
that count and at every larger one measured, is in `wins_from`; the routing in
modulate_sum.hip (modsum_route) is read off it.

Usage: python scripts/modulate_sum_time.py [--out profiles/modulate_sum_time.json] [--shapes abcd]
       [--warmup 100] [--steps 200] [--no-threshold]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

import srcdsp_amd as S
from carrier_sum_time import KINDS, SHAPES, SHIFT, timed, twice
from srcdsp_amd.design import hamming_sinc, q14

TILE = 2048
SCAN_L = {2: 32, 4: 128, 8: 64}  # L: taps
SCAN_C = (2, 8, 64)
SCAN_LG = tuple(range(4, 13))    # 16 .. 4096 tiles
SCAN_MAX_OUT = 1 << 30           # bytes of carrier rows at most


def chains(kind, C, L, ntaps):
    cls, _ = KINDS[kind]
    cq = q14(hamming_sinc(ntaps, 0.48 / L) * L / C)  # C carriers share the wire's range
    hs = [[], [], [], []]
    for c in range(C):
        m = S.Mixer(4096)
        m.reset(-0.9 + 1.8 * (c + 0.5) / C)
        for lst, h in zip(hs, (cls(), S.FilterUpsamplingFir(cq, L), S.QStagger(L // 2), m)):
            lst.append(h)
    return hs


def measure(kind, C, n, L, ntaps, warmup, steps, with_bank):
    _, bps = KINDS[kind]
    bits = torch.randint(0, 2, (C, bps * n), dtype=torch.uint8, device="cuda")
    rows = torch.empty((C, L * n, 2), dtype=torch.int16, device="cuda")
    wire = torch.empty((L * n, 2), dtype=torch.int16, device="cuda")
    wire2 = torch.empty_like(wire)
    hs = chains(kind, C, L, ntaps)

    def new(h=hs):
        S.modulate_sum_step(*h, bits, wire, SHIFT)

    def pair(h=hs):
        S.modulate_offset_step_batched(*h, bits, rows)
        S.combine(rows, wire2, SHIFT)

    def bank(h=hs):
        S.modulate_offset_step_batched(*h, bits, rows)

    # the same step from the same start on two sets of chains: the same wire
    s0 = S.modulate_sum_stats()
    new(chains(kind, C, L, ntaps))
    s1, b0 = S.modulate_sum_stats(), S.modulate_offset_stats()
    pair(chains(kind, C, L, ntaps))
    b1 = S.modulate_offset_stats()
    torch.cuda.synchronize()
    if not torch.equal(wire, wire2):
        raise SystemExit(f"{kind} C={C} n={n} L={L}: the new call and the pair disagree")
    path = ("fused kernel", "bank and combiner")[[b - a for a, b in zip(s0, s1)].index(1)]
    inner = ("fused kernel", "four operators", "bank launch", "per-channel loop")[[b - a for a, b in zip(b0, b1)].index(1)]
    fns = {"sum": new, "pair": pair}
    if with_bank:
        fns["bank"] = bank
    fns.update({k + "_again": v for k, v in list(fns.items())})
    ms = timed(fns, warmup, steps)
    new_t, new_spread = twice(ms, "sum")
    pair_t, pair_spread = twice(ms, "pair")
    r = {"kind": kind, "channels": C, "symbols_per_channel": n, "tiles": (n + TILE - 1) // TILE, "L": L, "D": L // 2,
         "ntaps": ntaps, "N": 4096, "shift": SHIFT, "sum_path": path, "pair_bank_path": inner,
         "ms_per_step": {k: round(v, 5) for k, v in ms.items()},
         "spread_ms": {"sum": round(new_spread, 5), "pair": round(pair_spread, 5)},
         "sum_over_pair": round(new_t / pair_t, 4),
         "sum_wins": bool(new_t < pair_t - pair_spread),  # by more than the pair's own spread
         "scratch_bytes_avoided": 4 * C * L * n}
    if with_bank:
        bank_t, bank_spread = twice(ms, "bank")
        r["spread_ms"]["bank"] = round(bank_spread, 5)
        r["bank_over_pair"] = round(bank_t / pair_t, 4)  # the bound: the pair without its combiner
    del bits, rows, wire, wire2
    torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modulate_sum_time.json"))
    ap.add_argument("--shapes", default="abcd")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--no-threshold", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("modulate_sum_time.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; the alternatives alternate per step, each timed twice; means; "
                       "the routing threshold at one tile for `sum`",
           "routing_in_the_library": {str(L): dict(zip(("min_tiles", "max_channels"), S.modulate_sum_geometry(L)[1:]))
                                      for L in (2, 4, 8)},
           "one_wire": {}, "threshold": {}}
    S.modulate_sum_set_min_tiles(1)
    try:
        for k in a.shapes:
            sh = SHAPES[k]
            for kind in KINDS:
                r = measure(kind, sh["C"], sh["n"], sh["L"], sh["ntaps"], a.warmup, a.steps, True)
                r["shape"] = f"{sh['name']}, D={sh['L'] // 2}"
                res["one_wire"][f"{k}_{kind}"] = r
        if not a.no_threshold:
            for L, ntaps in SCAN_L.items():
                for C in SCAN_C:
                    for lg in SCAN_LG:
                        n = TILE << lg
                        if 4 * C * L * n > SCAN_MAX_OUT:
                            continue
                        res["threshold"][f"L{L}_C{C}_2^{lg}"] = measure("qpsk", C, n, L, ntaps, a.warmup, a.steps, False)
            # per L and C: the smallest tile count from which the fused kernel wins at that count and at every
            # larger one measured (null: it does not win at the largest)
            rule = {}
            for L in SCAN_L:
                for C in SCAN_C:
                    pts = sorted((r["tiles"], r["sum_wins"]) for r in res["threshold"].values()
                                 if r["L"] == L and r["channels"] == C)
                    first = None
                    for tiles, wins in reversed(pts):
                        if not wins:
                            break
                        first = tiles
                    rule[f"L{L}_C{C}"] = {"wins_from_tiles": first, "largest_measured": pts[-1][0]}
            res["wins_from"] = rule
    finally:
        S.modulate_sum_set_min_tiles(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
