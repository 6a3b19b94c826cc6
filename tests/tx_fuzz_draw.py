"""The draws of the transmit fuzz (tests/test_gpu_fuzz.py:
test_fuzz_transmit_chain, test_fuzz_transmit_bank): shape, taps and operations
of a seed, from numpy alone, so that tests/test_tx_chain_model.py can replay
every seed without a GPU and hold the draws to their condition: most seeds on
the fused kernels, every family and kind present.

eligible() is the documented dispatch rule of the fused tiles (upmix.hip,
modulate.hip, modulate_offset.hip): variant 0, taps in int16 range,
2 <= L <= 8, at most 4096 taps, a mixer table of at most 4096 entries and, with
a stagger, D <= L; a call then takes the fused kernel when both its buffers
are 16-byte aligned, a bank when its row strides are multiples of 16 bytes
too."""
from __future__ import annotations

import numpy as np

import mapper_model as M
from tx_chain_model import FAMILIES, MODULATE_OFFSET, UPMIX

CHAIN_SEEDS, BANK_SEEDS = 36, 12
CHAIN_BASE, BANK_BASE = 10322, 11225
MAX_TAPS, MAX_N = 4096, 4096


def chain_rng(seed):
    return np.random.default_rng(CHAIN_BASE + seed)


def bank_rng(seed):
    return np.random.default_rng(BANK_BASE + seed)


def draw_taps(rng, L, H, variant, off=1.0):
    """(taps, what they are).  Full-range int16 mostly; a Q14 low-pass; the
    last L..2L taps zero (length < ntaps: a shorter flush); one tap of 1 << 20
    (variant 0 only: not the dot2 tap pairs)."""
    n = L * H
    u = rng.random()
    if u < 0.15 and n >= 2:
        from srcdsp_amd.design import hamming_sinc, q14  # numpy alone: the HIP library is not loaded
        return q14(hamming_sinc(n, 0.48 / L) * L), "q14"
    c = rng.integers(-32768, 32768, n).astype(np.int32)
    c[0], c[-1] = -32768, 32767
    if u < 0.30 and H >= 2:
        c[n - int(rng.integers(L, min(2 * L, n - L) + 1)):] = 0
        return c, "zero_tail"
    if u < 0.30 + 0.04 * off and variant == 0:
        c[int(rng.integers(0, n))] = 1 << 20
        return c, "wide"
    return c, "full"


def draw_shape(rng, off=1.0) -> dict:
    """off scales how often a trait the fused kernels do not take is drawn
    (L of 1 or 16, variant 1, a wide tap, N = 8192, D > L)."""
    family = FAMILIES[int(rng.integers(0, 3))]
    kind = None if family == UPMIX else int(rng.choice([M.SDPSK, M.QPSK]))
    L = int(rng.choice([1, 16])) if rng.random() < 0.06 * off else int(rng.integers(2, 9))
    H = int(rng.choice([1, 2, 5, 8, 16, 17, 32, 33, 64, 70]))
    variant = int(rng.random() < 0.05 * off)
    taps, taps_kind = draw_taps(rng, L, H, variant, off)
    p8192 = 0.05 * off
    N = int(rng.choice([4, 16, 1000, 1001, 4096, 8192], p=[0.15, 0.15, 0.2, 0.2, 0.3 - p8192, p8192]))
    D = None
    if family == MODULATE_OFFSET:
        u = rng.random()
        D = min(L + 1, 64) if u < 0.06 * off else (64 if u < 0.12 * off else int(rng.integers(1, L + 1)))
    return dict(family=family, kind=kind, L=L, H=H, variant=variant, taps=taps, taps_kind=taps_kind, N=N, D=D,
                freq=float(rng.uniform(-1, 1)), mapper_state=int(rng.integers(0, 4)))


def eligible(sh) -> bool:
    return (sh["variant"] == 0 and sh["taps_kind"] != "wide" and 2 <= sh["L"] <= 8 and sh["L"] * sh["H"] <= MAX_TAPS
            and sh["N"] <= MAX_N and (sh["D"] is None or sh["D"] <= sh["L"]))


def draw_size(rng):
    return int(rng.choice([0, 1, 3, 17, 511, 2048, 2049, int(rng.integers(0, 6000))]))


def draw_ops(rng, sh, n_ops=8):
    """The chain's operations in order: ("set_frequency", f),
    ("adjust_frequency", f), ("reset_mapper",), ("set_mapper_state", s),
    ("reset_stagger",), ("reset_up",), ("copy",), and ("step", dict(n=symbols or
    samples, flush, iterator, fused, off)) -- off: the input in a view one
    element off 16-byte alignment."""
    bits, stag = sh["family"] != UPMIX, sh["family"] == MODULATE_OFFSET
    ops = []
    for _ in range(n_ops):
        u = rng.random()
        if u < 0.08:
            ops.append(("set_frequency", float(rng.uniform(-1, 1))))
        elif u < 0.16:
            ops.append(("adjust_frequency", float(rng.uniform(-0.5, 0.5))))
        elif u < 0.22 and bits:
            ops.append(("reset_mapper",))
        elif u < 0.28 and bits:
            ops.append(("set_mapper_state", int(rng.integers(0, 4))))
        elif u < 0.34 and stag:
            ops.append(("reset_stagger",))
        elif u < 0.40:
            ops.append(("reset_up",))
        elif u < 0.50:
            ops.append(("copy",))
        n = draw_size(rng)
        ops.append(("step", dict(n=n, flush=bool(rng.random() < 0.2), iterator=bool(rng.random() < 0.2),
                                 fused=bool(rng.random() < 0.7), off=bool(n > 0 and rng.random() < 0.15))))
    return ops


def draw_input(rng, sh, n):
    """n symbols of bits (uint8 [n or 2n]) or n full-scale samples (int16 [n, 2])."""
    if sh["family"] == UPMIX:
        return rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    return rng.choice(np.array([0, 1, 2, 128, 255], np.uint8), n * (2 if sh["kind"] == M.QPSK else 1))


def draw_bank(rng) -> dict:
    """A bank seed: the shape (the traits off the fused kernels half as often
    as in a chain seed: the strides below take seeds off the bank kernel too),
    then rows, shared or per-row input, whether the input and output row
    strides are multiples of 16 bytes, and the calls (n, flush)."""
    sh = draw_shape(rng, off=0.5)
    sh["rows"] = int(rng.choice([1, 2, 5, 65]))
    sh["shared"] = bool(rng.random() < 0.35)
    sh["in_stride16"] = bool(rng.random() < 0.8)
    sh["out_stride16"] = bool(rng.random() < 0.8)
    sh["calls"] = [(int(rng.choice([0, 1, 17, 511, 2049, int(rng.integers(0, 2100))])), bool(rng.random() < 0.3))
                   for _ in range(3)]
    return sh


def bank_strides16(sh) -> bool:
    """Whether the bank's row strides leave it on the one-launch path (a
    shared input has stride 0)."""
    return (sh["shared"] or sh["in_stride16"]) and sh["out_stride16"]


def bank_eligible(sh) -> bool:
    return eligible(sh) and bank_strides16(sh)
