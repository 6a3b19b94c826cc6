"""Every instantiation of the fused transmit tile (up_dot2_tile in
up_dot2_kernels.h) against the oracle composition tests/tx_chain_model.py:

    upmix_tile_dot2<LR, PPC>       (upmix.hip)            samples -> up -> mixer
    modulate_tile_dot2<LR, PPC>    (modulate.hip)         bits -> mapper -> up -> mixer
    modoffset_tile_dot2<LR, PPC>   (modulate_offset.hip)  ... -> up -> stagger -> mixer

Each family dispatches on (L, PP = ceil(H / 2)), H taps per phase, to 15
kernels: PP compiled in at (L, PP) = (2,8) (2,16) (2,32) (4,8) (4,16) (4,32)
(8,8) (8,16), H at run time at L = 2..8; the stagger compiles one body per
delay D = 1..L into each.  The shape lists below name them all:

    COMPILED  (2,16) (2,32) (2,64) (4,16) (4,32) (4,64) (8,16) (8,32): the eight
              kernels; (2,15) (4,31) (8,31): the same PP with a padded last pair
    RUNTIME   (2,5) (3,9) (4,3) (5,7) (6,1) (7,11) (8,33): one per L, PP off
              the multiples of 4 and below 4; H = 1 has no history at all
    CEILING   (2,2048) (8,512): kUpMaxTaps = 4096 taps, the halo as long as a
              tile (interior at j0 - 8 HG = 0); (8,513): the pair / sequence path
    DELAYS    every (L, D), 2 <= L <= 8, 1 <= D <= L, at H = 3: the 35 bodies

Taps are full-range int16 with c[0] = -32768 and c[-1] = 32767 (upmix: with
full-scale input), so the int32 sums wrap and both clamps are reached.  Every
case is one chain whose state carries over calls of 4101 (a first, an interior
and a partial tile), 1, 513 (across a wave edge), 7 (less than a lane) with
flush and 0 with flush symbols or samples; after every call the output, the
mixer's (phase, word), the mapper state and the stagger carry equal the
model's bit for bit, the family's counters rose by exactly (1, 0, 0, 0) (the
fused kernel, not its fallback; (0, 1, 0, 0) for (8,513)) and the 24 samples
behind the output are untouched.  Nothing here is compared with another launch
of the tile."""
import numpy as np
import pytest

import mapper_model as M
from tx_chain_model import FAMILIES, MODULATE_OFFSET, UPMIX, TxChain
from tx_gpu import BIT_BYTES, GUARD_VALUE, GpuChain, bank_step, dev, stats_delta

pytestmark = pytest.mark.gpu

COMPILED = [(2, 16), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64), (8, 16), (8, 32), (2, 15), (4, 31), (8, 31)]
RUNTIME = [(2, 5), (3, 9), (4, 3), (5, 7), (6, 1), (7, 11), (8, 33)]
CEILING = [(2, 2048), (8, 512), (8, 513)]
SHAPES = COMPILED + RUNTIME + CEILING
MAX_TAPS = 4096
# the mixer of shape i: table sizes with N % 8 != 0 (1001, 4) and N < 8 (4) in every family
N_LIST = (4096, 1000, 1001, 16, 4)
FREQS = (0.1137, -0.3021, 0.73)
# the stagger's delay per shape, (SDPSK case, QPSK case): the compiled shapes of
# every L see D = 1, an odd D, L / 2 and L
DELAY = {(2, 16): (1, 2), (2, 32): (2, 1), (2, 64): (1, 2), (2, 15): (2, 1),
         (4, 16): (1, 4), (4, 32): (3, 2), (4, 64): (2, 3), (4, 31): (4, 1),
         (8, 16): (1, 8), (8, 32): (7, 4), (8, 31): (3, 8),
         (2, 5): (1, 2), (3, 9): (2, 3), (4, 3): (3, 1), (5, 7): (5, 2), (6, 1): (3, 6), (7, 11): (7, 4),
         (8, 33): (6, 2), (2, 2048): (2, 1), (8, 512): (5, 8), (8, 513): (3, 8)}
CALLS = [(4101, False), (1, False), (513, False), (7, True), (0, True)]
DELAY_CALLS = [(2053, False), (1, False), (5, True)]  # two tiles: the second's first lane takes D values of the halo
WARM = 100
KIND_NAME = {None: "", M.SDPSK: "-sdpsk", M.QPSK: "-qpsk"}
FUSED, FALLBACK, BANK = (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0)


def kinds(family):
    return (None,) if family == UPMIX else (M.SDPSK, M.QPSK)


def full_taps(L, H):
    c = np.random.default_rng(1000 * L + H).integers(-32768, 32768, L * H).astype(np.int32)
    c[0], c[-1] = -32768, 32767
    return c


def inputs(O, family, kind, n, seed, row=0):
    """n symbols of bits, or n full-scale samples."""
    if family == UPMIX:
        return O["strict"].gen_ci16(0x7A5 + seed, row, 0, n, -32768, 32767)
    return np.random.default_rng(1000 * seed + row).choice(BIT_BYTES, n * (2 if kind == M.QPSK else 1))


def pair(S, O, family, kind, L, H, N, f, D, state=3):
    c = full_taps(L, H)
    return (GpuChain(S, family, L, c, N, f, kind, D, mapper_state=state),
            TxChain(O["strict"], family, L, c, N, f, kind, D, mapper_state=state))


def same(y, want, what):
    y, want = np.asarray(y).reshape(-1, 2), np.asarray(want).reshape(-1, 2)
    assert y.shape == want.shape, what
    bad = np.flatnonzero((y != want).any(1))
    assert bad.size == 0, (what, "first output index", int(bad[0]), y[bad[0]].tolist(), want[bad[0]].tolist(),
                           "differing", int(bad.size), "of", len(y))


def warm_up(O, g, m, family, kind):
    """A history, a phase, a mapper state and a carry to start from."""
    x = inputs(O, family, kind, WARM, 1)
    same(g.separate(dev(x)).cpu().numpy(), m.step(x), "warm-up")
    assert g.state() == m.state()


def run_calls(O, g, m, family, kind, calls, want):
    for k, (n, flush) in enumerate(calls):
        x = inputs(O, family, kind, n, 10 + k)
        xd = dev(x)  # an allocation of its own: 16-byte aligned
        ref = m.step(x, flush)
        assert len(ref) == g.n_out(len(x), flush) and len(ref) > 0
        buf = g.guarded(len(ref))
        _, d = stats_delta(g, lambda: g.fused(xd, flush, False, buf[:len(ref)]))
        assert d == want, (k, d)
        y = buf.cpu().numpy()
        same(y[:len(ref)], ref, ("call", k, n, flush))
        assert (y[len(ref):] == GUARD_VALUE).all(), k
        assert g.state() == m.state(), k
    # the interpolator's history: a further flushing step on copies
    g2, m2 = g.copy(), m.copy()
    x = inputs(O, family, kind, 40, 99)
    same(g2.separate(dev(x), True).cpu().numpy(), m2.step(x, True), "history")
    assert g2.state() == m2.state()


def sweep_cases():
    for family in FAMILIES:
        for i, (L, H) in enumerate(SHAPES):
            for kind in kinds(family):
                D = DELAY[(L, H)][kind == M.QPSK] if family == MODULATE_OFFSET else None
                ident = f"{family}-L{L}xH{H}{KIND_NAME[kind]}" + (f"-D{D}" if D else "")
                yield pytest.param(family, kind, L, H, N_LIST[i % len(N_LIST)], FREQS[i % len(FREQS)], D, id=ident)


@pytest.mark.parametrize("family,kind,L,H,N,f,D", list(sweep_cases()))
def test_instantiation_vs_oracle(S, O, family, kind, L, H, N, f, D):
    g, m = pair(S, O, family, kind, L, H, N, f, D)
    warm_up(O, g, m, family, kind)
    run_calls(O, g, m, family, kind, CALLS, FUSED if L * H <= MAX_TAPS else FALLBACK)


def delay_cases():
    i = 0
    for L in range(2, 9):
        for D in range(1, L + 1):
            for kind in (M.SDPSK, M.QPSK):
                yield pytest.param(kind, L, D, N_LIST[i % len(N_LIST)], FREQS[i % len(FREQS)],
                                   id=f"L{L}-D{D}{KIND_NAME[kind]}")
            i += 1


@pytest.mark.parametrize("kind,L,D,N,f", list(delay_cases()))
def test_stagger_delay_vs_oracle(S, O, kind, L, D, N, f):
    g, m = pair(S, O, MODULATE_OFFSET, kind, L, 3, N, f, D)
    warm_up(O, g, m, MODULATE_OFFSET, kind)
    run_calls(O, g, m, MODULATE_OFFSET, kind, DELAY_CALLS, FUSED)


# a compiled L = 8 kernel and a run-time odd-L kernel per family (the batch split
# at 65 rows is covered at L = 4 by the families' own bank tests)
@pytest.mark.parametrize("L,H,kind,D", [(8, 16, M.QPSK, 8), (5, 7, M.SDPSK, 3)], ids=["L8xH16", "L5xH7"])
@pytest.mark.parametrize("family", FAMILIES)
def test_bank_vs_oracle(S, O, family, L, H, kind, D):
    """3 rows with their own input, mapper state, history, carry and carrier
    in one launch, every row against its own model chain."""
    import torch
    rows = 3
    kind = None if family == UPMIX else kind
    ps = [pair(S, O, family, kind, L, H, 1000, FREQS[r] * 0.5, D if family == MODULATE_OFFSET else None, state=r + 1)
          for r in range(rows)]
    for r, (g, m) in enumerate(ps):
        x = inputs(O, family, kind, 20 + r, 1, r)
        same(g.separate(dev(x)).cpu().numpy(), m.step(x), "warm-up")
        assert g.state() == m.state(), r
    chains = [g for g, _ in ps]
    for k, (n_sym, flush) in enumerate([(2055, False), (9, True)]):
        xs = [inputs(O, family, kind, n_sym, 10 + k, r) for r in range(rows)]
        n = len(xs[0])
        stride = (n + 15) // 16 * 16  # elements: rows 16-byte aligned for bits and for samples
        host = np.zeros((rows, stride) + xs[0].shape[1:], xs[0].dtype)
        host[:, :n] = np.stack(xs)
        refs = [m.step(x, flush) for (_, m), x in zip(ps, xs)]
        n_out = len(refs[0])
        out = torch.full((rows, (n_out + 24 + 3) // 4 * 4, 2), GUARD_VALUE, dtype=torch.int16, device="cuda")
        xd = dev(host)
        _, d = stats_delta(chains[0], lambda: bank_step(chains, xd, stride, out, n, flush))
        assert d == BANK, (k, d)
        y = out.cpu().numpy()
        assert (y[:, n_out:] == GUARD_VALUE).all(), k
        for r, (g, m) in enumerate(ps):
            same(y[r, :n_out], refs[r], ("call", k, "row", r))
            assert g.state() == m.state(), (k, r)
    for r, (g, m) in enumerate(ps):  # every row's history: a further flushing step on copies
        x = inputs(O, family, kind, 40, 99, r)
        g2, m2 = g.copy(), m.copy()
        same(g2.separate(dev(x), True).cpu().numpy(), m2.step(x, True), ("history", r))
        assert g2.state() == m2.state(), r
