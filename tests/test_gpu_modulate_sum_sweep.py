"""Every instantiation of the summing transmit tile (modsum_tile_dot2,
modulate_sum.hip) against the model: tx_chain_model.TxChain rows combined by
combine_model.combine.  The launcher dispatches on L in {2, 4, 8}, on PP =
ceil(H / 2) (compiled in at 8 and, below L = 8, at 16 and 32; else H at run
time) and on whether the chains have a stagger: 20 kernels.  The shapes (L, H)
name them all, each run with and without staggers:

    L = 2: 16 32 64 | 15 | 5 | 2048     PP 8, 16, 32; a padded last pair; run-time; kUpMaxTaps
    L = 4: 16 32 64 | 31 | 3
    L = 8: 16 | 15 | 32 31 64 33 | 512  PP 8; padded; run-time (PP 16 and 32 have no compiled kernel at L = 8); kUpMaxTaps

(This sweep found modsum_tile_dot2<8, 16, stagger on and off> wrong on hardware
at (8,32) and (8,31): all but 16..40 of the 32 808 samples of the first call
differed from the model.  The launcher now sends PP = 16 at L = 8 to the
run-time kernel, which these two shapes hold to the model.)

Every case is 3 chains with their own frequency, mapper state, warm-up history
and carry, stepped over the calls of the transmit sweep (4101: a first, an
interior and a partial tile; 1; 513; 7 with flush; 0 with flush).  After every
call the wire equals the model's bit for bit, each chain's mapper state, mixer
(phase, word) and stagger carry equal its model chain's, the counters rose by
exactly (1, 0) and the 24 samples behind the row are untouched; at the end the
interpolators' histories are compared through a flushing step on copies.  The
mapper kinds alternate over the list; with staggers D cycles 1..L at L = 2 and
4 and is 4 at L = 8, the delay that kernel compiles in (one more case, L = 8
with D = 3, must go to the bank and the combiner and equal the model too).  Taps
are full-range int16; the combiner's shift cycles 0..2, so that the wire sits
on the int16 clamp in some cases of every L and in others nowhere
(test_the_wire_clamps_in_some_cases_and_not_in_others).  Nothing here is
compared with another GPU launch."""
import numpy as np
import pytest

import mapper_model as M
from combine_model import combine as combine_model
from test_gpu_modulate_sum import every_tile_count, stats_delta, sum_call  # noqa: F401  (a fixture)
from test_gpu_tx_sweep import CALLS, FREQS, KIND_NAME, N_LIST, full_taps, inputs, same
from tx_chain_model import MODULATE, MODULATE_OFFSET, TxChain
from tx_gpu import GUARD, GUARD_VALUE, GpuChain, dev

gpu = pytest.mark.gpu

SHAPES = [(2, 16), (2, 32), (2, 64), (2, 15), (2, 5), (2, 2048),
          (4, 16), (4, 32), (4, 64), (4, 31), (4, 3),
          (8, 16), (8, 15), (8, 32), (8, 31), (8, 64), (8, 33), (8, 512)]
ROWS, WARM, MAX_TAPS = 3, 100, 4096
FUSED, BANK = (1, 0), (0, 1)


def cases():
    """(L, H, stagger, kind, D, shift, N, want)"""
    out = []
    for i, (L, H) in enumerate(SHAPES):
        j = [s for s in SHAPES if s[0] == L].index((L, H))
        for stagger in (True, False):
            kind = (M.SDPSK, M.QPSK)[(i + stagger) % 2]
            D = (4 if L == 8 else 1 + j % L) if stagger else None
            out.append((L, H, stagger, kind, D, (i + 2 * stagger) % 3, N_LIST[i % len(N_LIST)], FUSED))
    out.append((8, 16, True, M.QPSK, 3, 1, 1000, BANK))  # not the delay the L = 8 kernel compiles in
    return out


CASES = cases()


def ident(c):
    L, H, stagger, kind, D, shift, N, _ = c
    return f"L{L}xH{H}{KIND_NAME[kind]}-" + (f"D{D}" if stagger else "plain") + f"-s{shift}-N{N}"


def kernel_of(L, H, stagger):
    """The instantiation <LR, PPC, STG> sum_fused (modulate_sum.hip) picks."""
    PP = (H + 1) // 2
    return L, PP if PP == 8 or (PP in (16, 32) and L < 8) else 0, stagger


def test_the_sweep_covers_what_it_names():
    fused = [c for c in CASES if c[7] == FUSED]
    assert all(c[0] in (2, 4, 8) and c[0] * c[1] <= MAX_TAPS and c[5] in (0, 1, 2) for c in CASES)
    assert all(c[4] is None or (c[4] <= c[0] and (c[0] != 8 or c[4] == 4)) for c in fused)  # what fused_takes asks of D
    every = {(L, PP, s) for L in (2, 4, 8) for PP in (8, 16, 32, 0) for s in (True, False)
             if (L, PP) not in ((8, 16), (8, 32))}
    assert len(every) == 20 and {kernel_of(c[0], c[1], c[2]) for c in fused} == every
    assert {(c[0], c[1]) for c in fused} >= {(8, 32), (8, 31)}  # where the compiled kernel was wrong
    for L in (2, 4, 8):
        mine = [c for c in fused if c[0] == L]
        # a compiled PP with a padded last pair, run-time taps off a multiple of 4 pairs, the ceiling
        assert any(c[1] % 2 and kernel_of(L, c[1], True)[1] for c in mine)
        assert any(kernel_of(L, c[1], True)[1] == 0 and ((c[1] + 1) // 2) % 4 for c in mine)
        for stagger in (True, False):  # both kinds with and without staggers
            assert {c[3] for c in mine if c[2] == stagger} == {M.SDPSK, M.QPSK}, (L, stagger)
        assert {c[4] for c in mine if c[2]} == ({4} if L == 8 else set(range(1, L + 1))), L
        assert {c[5] for c in mine} == {0, 1, 2}
    assert {(c[0], c[1]) for c in fused} >= {(2, 2048), (8, 512)}
    extra = [c for c in CASES if c[7] == BANK]
    assert [(c[0], c[2], c[4]) for c in extra] == [(8, True, 3)]
    assert [n for n, _ in CALLS] == [4101, 1, 513, 7, 0] and [f for _, f in CALLS] == [False, False, False, True, True]


def freqs(case):
    i = CASES.index(case)
    return [FREQS[(i + r) % len(FREQS)] * (0.5 if r == 1 else 1.0) for r in range(ROWS)]


def row_bits(O, case, n_sym, seed):
    _, _, stagger, kind, _, _, _, _ = case
    return [inputs(O, MODULATE_OFFSET if stagger else MODULATE, kind, n_sym, seed, r) for r in range(ROWS)]


_MODEL = {}


def model(O, case):
    """The model's run of a case, once: the rows' warm-up outputs; per call the
    wire and every chain's state; the rows' outputs and states of a further
    flushing step on copies (the interpolators' histories)."""
    if case not in _MODEL:
        L, H, stagger, kind, D, shift, N, _ = case
        family = MODULATE_OFFSET if stagger else MODULATE
        c = full_taps(L, H)
        chains = [TxChain(O["strict"], family, L, c, N, f, kind, D, mapper_state=r + 1)
                  for r, f in enumerate(freqs(case))]
        warm = [m.step(row_bits(O, case, WARM + 7 * r, 1)[r]) for r, m in enumerate(chains)]
        warm_states = [m.state() for m in chains]
        calls = []
        for k, (n, flush) in enumerate(CALLS):
            bits = row_bits(O, case, n, 10 + k)
            wire = combine_model(np.stack([m.step(b, flush) for m, b in zip(chains, bits)]), shift)
            calls.append((wire, [m.state() for m in chains]))
        copies = [m.copy() for m in chains]
        tail = [m.step(b, True) for m, b in zip(copies, row_bits(O, case, 40, 99))]
        _MODEL[case] = dict(warm=warm, warm_states=warm_states, calls=calls, tail=tail,
                            tail_states=[m.state() for m in copies])
    return _MODEL[case]


def clamp_share(ref):
    y = np.concatenate([w for w, _ in ref["calls"]]).astype(np.int32)
    return float(np.mean((y == 32767) | (y == -32768)))


@pytest.mark.parametrize("L", [2, 4, 8])
def test_the_wire_clamps_in_some_cases_and_not_in_others(O, L):
    """A condition on the model alone: the combiner's clamp and its shift are
    both exercised at every L."""
    clamped = clear = None
    for case in (c for c in CASES if c[0] == L and c[1] <= 64):
        share = clamp_share(model(O, case))
        print(f"{ident(case)}: share of the model's wire on the int16 clamp {share:.4f}")
        if share >= 0.05:
            clamped = case
        if share == 0.0:
            clear = case
        if clamped and clear:
            break
    assert clamped and clear, (L, clamped, clear)


@gpu
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_instantiation_vs_model(S, O, every_tile_count, case):
    import torch
    L, H, stagger, kind, D, shift, N, want = case
    family = MODULATE_OFFSET if stagger else MODULATE
    ref = model(O, case)
    c = full_taps(L, H)
    chains = [GpuChain(S, family, L, c, N, f, kind, D, mapper_state=r + 1) for r, f in enumerate(freqs(case))]
    for r, g in enumerate(chains):  # a history, a phase, a mapper state and a carry of its own
        same(g.separate(dev(row_bits(O, case, WARM + 7 * r, 1)[r])).cpu().numpy(), ref["warm"][r], ("warm-up", r))
        assert g.state() == ref["warm_states"][r], r
    for k, (n, flush) in enumerate(CALLS):
        bits = row_bits(O, case, n, 10 + k)
        n_bits = len(bits[0])
        stride = max((n_bits + 15) // 16 * 16, 16)  # private rows a multiple of 16 bytes apart
        host = np.zeros((ROWS, stride), np.uint8)
        host[:, :n_bits] = np.stack(bits)
        wire, states = ref["calls"][k]
        out = torch.full((len(wire) + GUARD, 2), GUARD_VALUE, dtype=torch.int16, device="cuda")
        bd = dev(host)
        # sum_call checks the samples behind the row
        y, d = stats_delta(S, lambda: sum_call(S, chains, bd, stride, n_bits, flush, shift, stagger, out=out,
                                               n_out=len(wire)))
        assert d == want, (k, d)
        same(y, wire, ("call", k, n, flush))
        for r, g in enumerate(chains):
            assert g.state() == states[r], (k, r)
    for r, g in enumerate(chains):  # the interpolator's history: a further flushing step on copies
        g2 = g.copy()
        same(g2.separate(dev(row_bits(O, case, 40, 99)[r]), True).cpu().numpy(), ref["tail"][r], ("history", r))
        assert g2.state() == ref["tail_states"][r], r
