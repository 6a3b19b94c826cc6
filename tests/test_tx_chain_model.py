"""The yardstick of the transmit sweep and fuzz held to the reference without
a GPU: tx_chain_model.TxChain replays every chain golden recorded from the
reference build (chain_* of mapper_golden.npz: mapper -> FilterUpsamplingFir ->
Mixer; every chain of oqpsk_golden.npz: the same with the Q-rail stagger) bit
for bit, its copies continue a stream like the original, and the draws of the
transmit fuzz (tx_fuzz_draw) stay on the fused kernels."""
import collections

import numpy as np
import pytest

import mapper_model as M
import stagger_model as G
import tx_fuzz_draw as F
from tx_chain_model import MODULATE, MODULATE_OFFSET, UPMIX, TxChain

MAN_M, ARR_M = M.load_golden()
MAN_G, ARR_G = G.load_golden()


def replay(O, family, chain, arr):
    k = chain["key"]
    ch = TxChain(O["strict"], family, chain["L"], arr[k + "_taps"], chain["N"], chain["freq"], kind=chain["kind"],
                 D=chain.get("D"))
    bits, pos, ys = arr[k + "_bits"], 0, []
    for n, flush in zip(chain["calls"], chain["flush"]):
        ys.append(ch.step(bits[pos:pos + n], flush))
        assert len(ys[-1]) == ch.n_out(n, flush)
        pos += n
    return ch, np.concatenate(ys)


@pytest.mark.parametrize("chain", MAN_M["chains"], ids=[c["key"] for c in MAN_M["chains"]])
def test_modulate_goldens(O, chain):
    ch, y = replay(O, MODULATE, chain, ARR_M)
    k = chain["key"]
    assert np.array_equal(y, ARR_M[k + "_out"])
    # this manifest records no final state: the mapper's against the reference's loops restated
    # (mapper_model.step_loop), the mixer's phase against mixers.h:177 in closed form
    st = ch.state()
    assert st["mapper"] == M.step_loop(chain["kind"], 0, ARR_M[k + "_bits"])[1]
    phase, word = st["mixer"]
    assert phase == len(y) * word % chain["N"]


@pytest.mark.parametrize("chain", MAN_G["chains"], ids=[c["key"] for c in MAN_G["chains"]])
def test_modulate_offset_goldens(O, chain):
    ch, y = replay(O, MODULATE_OFFSET, chain, ARR_G)
    k = chain["key"]
    assert np.array_equal(y, ARR_G[k + "_out"])
    st = ch.state()
    assert st["mapper"] == chain["mapper_state"] and st["carry"] == ARR_G[k + "_carry"].tolist()
    assert st["mixer"][0] == chain["mixer_phase"]


def test_upmix_is_the_two_oracle_calls(O):
    """No golden has samples for input: the family is the oracle's
    interpolator and mixer (tests/test_oracle_golden.py) and nothing else."""
    o = O["strict"]
    c = np.random.default_rng(1).integers(-32768, 32768, 4 * 9)
    x = o.gen_ci16(7, 0, 0, 300, -32768, 32767)
    ch = TxChain(o, UPMIX, 4, c, 1000, 0.3)
    up, mixer = o.up(0, 4, c), o.mixer(1000)
    mixer.reset(0.3)
    for a, b, flush, it in ((0, 100, False, False), (100, 100, False, True), (100, 300, True, False)):
        assert np.array_equal(ch.step(x[a:b], flush, it), mixer.step(up.step(x[a:b], flush, it)))
        assert ch.state() == {"mixer": tuple(mixer.state()[:2])}


@pytest.mark.parametrize("seed", range(F.CHAIN_SEEDS))
def test_copies_continue_the_stream(O, seed):
    """Every drawn chain with a copy taken before each step: the copy's step
    is the original's, outputs and state."""
    rng = F.chain_rng(seed)
    sh = F.draw_shape(rng)
    ops = F.draw_ops(rng, sh)
    ch = TxChain(O["strict"], sh["family"], sh["L"], sh["taps"], sh["N"], sh["freq"], kind=sh["kind"], D=sh["D"],
                 variant=sh["variant"], mapper_state=sh["mapper_state"])
    for op in ops:
        if op[0] == "copy":
            ch = ch.copy()
        elif op[0] != "step":
            getattr(ch, op[0])(*op[1:])
        else:
            a = op[1]
            x = F.draw_input(rng, sh, min(a["n"], 300))
            twin = ch.copy()
            assert twin.state() == ch.state()
            y = ch.step(x, a["flush"], a["iterator"])
            assert np.array_equal(twin.step(x, a["flush"], a["iterator"]), y)
            assert twin.state() == ch.state()
            assert len(y) == ch.n_out(len(x), a["flush"])


def test_fuzz_draws_stay_on_the_fused_kernels():
    """At least two thirds of the chain seeds and of the bank seeds draw a
    shape the fused kernels take (the bank seeds with strides the bank kernel
    takes, too); every family and kind occurs in at least three chain seeds."""
    shapes = [F.draw_shape(F.chain_rng(s)) for s in range(F.CHAIN_SEEDS)]
    assert 3 * sum(F.eligible(sh) for sh in shapes) >= 2 * len(shapes)
    seen = collections.Counter((sh["family"], sh["kind"]) for sh in shapes)
    for key in [(UPMIX, None)] + [(f, k) for f in (MODULATE, MODULATE_OFFSET) for k in (M.SDPSK, M.QPSK)]:
        assert seen[key] >= 3, (key, seen)
    banks = [F.draw_bank(F.bank_rng(s)) for s in range(F.BANK_SEEDS)]
    assert 3 * sum(F.eligible(sh) for sh in banks) >= 2 * len(banks)
    assert 3 * sum(F.bank_eligible(sh) for sh in banks) >= 2 * len(banks)


def test_fuzz_draws_reach_what_they_are_for():
    """Every path prediction of the fuzz has a seed: a change of weights or of
    a seed base cannot silently remove one."""
    shapes = [F.draw_shape(F.chain_rng(s)) for s in range(F.CHAIN_SEEDS)]
    steps = [op[1] for s in range(F.CHAIN_SEEDS) for op in _ops(s) if op[0] == "step"]
    assert any(a["flush"] and a["n"] == 0 for a in steps) and any(a["off"] for a in steps)
    assert any(not a["fused"] for a in steps) and any(a["iterator"] for a in steps)
    assert {sh["taps_kind"] for sh in shapes} == {"full", "q14", "zero_tail", "wide"}
    # each trait the fused kernels do not take, in a chain seed
    assert any(sh["D"] == 64 for sh in shapes)
    assert any(sh["D"] is not None and sh["D"] == sh["L"] + 1 for sh in shapes)
    assert any(sh["L"] in (1, 16) for sh in shapes)
    assert any(sh["variant"] == 1 for sh in shapes)
    assert any(sh["N"] == 8192 for sh in shapes)
    for op in ("set_frequency", "adjust_frequency", "reset_mapper", "set_mapper_state", "reset_stagger", "reset_up",
               "copy"):
        assert any(o[0] == op for s in range(F.CHAIN_SEEDS) for o in _ops(s)), op
    # banks: both paths for every family, the loop for a shape and for either stride alone (on a shape
    # the bank kernel would take, with more than one row and a call that has output)
    banks = [F.draw_bank(F.bank_rng(s)) for s in range(F.BANK_SEEDS)]
    runs = lambda sh: sh["rows"] > 1 and any(n > 0 for n, _ in sh["calls"])  # noqa: E731
    for family in (UPMIX, MODULATE, MODULATE_OFFSET):
        assert sum(F.bank_eligible(sh) for sh in banks if sh["family"] == family) >= 2, family
    assert any(not F.eligible(sh) for sh in banks)
    assert any(F.eligible(sh) and runs(sh) and not sh["shared"] and not sh["in_stride16"] and sh["out_stride16"]
               for sh in banks)
    assert any(F.eligible(sh) and runs(sh) and (sh["shared"] or sh["in_stride16"]) and not sh["out_stride16"]
               for sh in banks)
    assert any(F.bank_eligible(sh) and sh["shared"] for sh in banks)
    assert any(F.bank_eligible(sh) and not sh["shared"] for sh in banks)
    assert {sh["rows"] for sh in banks} == {1, 2, 5, 65}
    assert any(n == 0 and flush for sh in banks for n, flush in sh["calls"])


def _ops(seed):
    rng = F.chain_rng(seed)
    return F.draw_ops(rng, F.draw_shape(rng))
