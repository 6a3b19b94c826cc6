"""The draws of the resampler fuzz (tests/test_gpu_fuzz.py:
test_fuzz_resample_chain, test_fuzz_resample_bank): shape, taps and operations
of a seed, from numpy alone, so that tests/test_resample_fuzz_draw.py can
replay every seed without a GPU and hold the draws to their conditions.

eligible() restates fused_takes of resample.hip: interpolator variant 0 with
int16-range taps, 2 <= L <= 8, at most 4096 taps; decimator variant 1 with
int16-range taps, 1 <= M <= 8, at most 1024 taps.  A call of such a shape takes
the fused kernel when both its buffers are 16-byte aligned, a bank its one
launch when its row strides are multiples of 16 bytes too (the tests run under
resample_set_min_tiles(1): every call the kernel takes goes to it)."""
from __future__ import annotations

import math

import numpy as np

CHAIN_SEEDS, BANK_SEEDS = 36, 12
CHAIN_BASE, BANK_BASE = 20065, 21000  # bases at which tests/test_resample_fuzz_draw.py's conditions hold
MAX_UP_TAPS, MAX_DECIM_TAPS = 4096, 1024
H_LIST = (1, 2, 5, 8, 16, 17, 32, 33, 64, 70)
ND_LIST = (1, 2, 3, 7, 8, 9, 31, 63, 64, 96, 127, 128, 255, 256, 1000, 1024, 1025)
TAPS_KINDS = ("full", "dense", "zero_tail", "wide")


def chain_rng(seed):
    return np.random.default_rng(CHAIN_BASE + seed)


def bank_rng(seed):
    return np.random.default_rng(BANK_BASE + seed)


def draw_taps(rng, kind, n, zero_lo, wide_ok):
    """n taps of a kind.  "full": full-range int16 with both extremes at the
    ends; "dense": none zero, +-32767 at the ends; "zero_tail": full with the
    last zero_lo..2 zero_lo taps zero (an interpolator's length < ntaps: a
    shorter flush) where n allows; "wide": full with one tap of 1 << 20 (beyond
    int16: not the dot2 tap pairs) where the variant holds it."""
    if kind == "dense":
        c = (rng.integers(1, 32768, n) * rng.choice([-1, 1], n)).astype(np.int32)
        c[-1], c[0] = -32767, 32767
        return c
    c = rng.integers(-32768, 32768, n).astype(np.int32)
    c[-1], c[0] = 32767, -32768
    if kind == "zero_tail" and n >= 2 * zero_lo:
        c[n - int(rng.integers(zero_lo, min(2 * zero_lo, n - zero_lo) + 1)):] = 0
    if kind == "wide" and wide_ok:
        c[int(rng.integers(0, n))] = 1 << 20
    return c


def up_length(c):
    """FilterUpsamplingFir::length: the taps without their trailing zeros."""
    nz = np.flatnonzero(c)
    return int(nz[-1]) + 1 if nz.size else 0


def draw_shape(rng, off=1.0) -> dict:
    """off scales how often a trait the fused kernel does not take is drawn (L
    of 1, 9 or 16, M of 12 or 16, interpolator variant 1, decimator variant 2,
    a wide tap, N_d = 1025)."""
    L = int(rng.choice([1, 9, 16])) if rng.random() < 0.06 * off else int(rng.integers(2, 9))
    M = int(rng.choice([12, 16])) if rng.random() < 0.06 * off else int(rng.integers(1, 9))
    H = int(rng.choice(H_LIST))
    p_over = 0.06 * off  # N_d = 1025, above the cap
    Nd = int(rng.choice(ND_LIST, p=[(1 - p_over) / (len(ND_LIST) - 1)] * (len(ND_LIST) - 1) + [p_over]))
    uvar = int(rng.random() < 0.05 * off)
    dvar = 2 if rng.random() < 0.05 * off else 1
    p_wide = 0.08 * off
    kind = str(rng.choice(TAPS_KINDS, p=[0.45 - p_wide, 0.30, 0.25, p_wide]))
    wide_up = bool(rng.random() < 0.5)  # which filter has the wide tap
    cu = draw_taps(rng, kind, L * H, L, uvar == 0 and wide_up)
    cd = draw_taps(rng, kind, Nd, 1, dvar == 1 and not (uvar == 0 and wide_up))
    return dict(L=L, M=M, H=H, Nd=Nd, uvar=uvar, dvar=dvar, taps_kind=kind, cu=cu, cd=cd,
                ls=int(rng.integers(0, 4)), g=M // math.gcd(L, M), flush_inputs=up_length(cu) // L)


def int16_range(c) -> bool:
    return bool(c.min() >= -32768 and c.max() <= 32767)


def eligible(sh) -> bool:
    return (sh["uvar"] == 0 and int16_range(sh["cu"]) and 2 <= sh["L"] <= 8 and sh["L"] * sh["H"] <= MAX_UP_TAPS
            and sh["dvar"] == 1 and int16_range(sh["cd"]) and 1 <= sh["M"] <= 8 and sh["Nd"] <= MAX_DECIM_TAPS)


def legal(sh, n, flush):
    """The nearest length >= about n the call accepts: L (n + length / L when
    flushing) a multiple of M, which is n (+ length / L) a multiple of g."""
    g = sh["g"]
    n = n // g * g
    return n + (-(n + sh["flush_inputs"])) % g if flush else n


def draw_ops(rng, sh, n_ops=8):
    """The chain's operations in order: ("set_left_shift", ls), ("reset_up",),
    ("reset_decim",), ("copy",) and ("step", dict(n, flush, fused, off)) --
    fused: the one call, else the two single operators on the same handles; off:
    the input in a view one sample off 16-byte alignment."""
    g = sh["g"]
    ops = []
    for _ in range(n_ops):
        u = rng.random()
        if u < 0.10:
            ops.append(("set_left_shift", int(rng.integers(0, 4))))
        elif u < 0.17:
            ops.append(("reset_up",))
        elif u < 0.24:
            ops.append(("reset_decim",))
        elif u < 0.34:
            ops.append(("copy",))
        flush = bool(rng.random() < 0.2)
        n = legal(sh, int(rng.choice([0, g, 3 * g, 2048, 2049, int(rng.integers(0, 6001))])), flush)
        ops.append(("step", dict(n=n, flush=flush, fused=bool(rng.random() < 0.7),
                                 off=bool(n > 0 and rng.random() < 0.15))))
    return ops


def draw_input(rng, n):
    """n full-scale samples (int16 [n, 2])."""
    return rng.integers(-32768, 32768, (n, 2)).astype(np.int16)


def draw_bank(rng) -> dict:
    """A bank seed: the shape (the traits off the fused kernel half as often as
    in a chain seed: the strides below take seeds off the one launch too), then
    rows, whether the input and output row strides are multiples of 16 bytes,
    and the calls (n, flush)."""
    sh = draw_shape(rng, off=0.5)
    sh["rows"] = int(rng.choice([1, 2, 5, 65]))
    sh["in_stride16"] = bool(rng.random() < 0.8)
    sh["out_stride16"] = bool(rng.random() < 0.8)
    g = sh["g"]
    sh["calls"] = []
    for _ in range(3):
        flush = bool(rng.random() < 0.3)
        n = int(rng.choice([0, g, 17, 511, 2049, int(rng.integers(0, 2100))]))
        sh["calls"].append((legal(sh, n, flush), flush))
    return sh


def bank_eligible(sh) -> bool:
    """Whether the bank stays on its one-launch path."""
    return eligible(sh) and sh["in_stride16"] and sh["out_stride16"]
