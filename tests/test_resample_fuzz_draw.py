"""The draws of the resampler fuzz (tests/resample_fuzz_draw.py) replayed
without a GPU and held to their conditions: most chain seeds on the fused
kernel, every L and M it takes among them, the edges of its call plan (a flush,
a step shorter than the interpolator's history, a step with L n < N_d - 1), and
banks on the one-launch path.  A change of weights or of a seed base cannot
silently remove one."""
import resample_fuzz_draw as F


def _chain(seed):
    rng = F.chain_rng(seed)
    sh = F.draw_shape(rng)
    return sh, F.draw_ops(rng, sh)


CHAINS = [_chain(s) for s in range(F.CHAIN_SEEDS)]
BANKS = [F.draw_bank(F.bank_rng(s)) for s in range(F.BANK_SEEDS)]


def _steps(ops):
    return [op[1] for op in ops if op[0] == "step"]


def test_every_drawn_call_is_legal():
    for sh, ops in CHAINS:
        assert len(sh["cu"]) == sh["L"] * sh["H"] and len(sh["cd"]) == sh["Nd"]
        assert sh["flush_inputs"] == F.up_length(sh["cu"]) // sh["L"] and sh["cu"][0] != 0
        for a in _steps(ops):
            assert a["n"] >= 0 and (sh["L"] * (a["n"] + (sh["flush_inputs"] if a["flush"] else 0))) % sh["M"] == 0
    for sh in BANKS:
        for n, flush in sh["calls"]:
            assert 0 <= n <= 2100 + sh["g"] and (sh["L"] * (n + (sh["flush_inputs"] if flush else 0))) % sh["M"] == 0


def test_chain_draws_stay_on_the_fused_kernel_and_reach_its_edges():
    fused = [(sh, ops) for sh, ops in CHAINS if F.eligible(sh)]
    assert 10 * len(fused) >= 6 * len(CHAINS), len(fused)
    assert {sh["L"] for sh, _ in fused} == set(range(2, 9))
    assert {sh["M"] for sh, _ in fused} == set(range(1, 9))
    assert any(sh["M"] % 2 and sh["M"] > 1 and sh["L"] % 2 for sh, _ in fused)
    # on the fused kernel: a call served by it (not in a view off 16 bytes, with output) ...
    calls = [(sh, a) for sh, ops in fused for a in _steps(ops) if a["fused"] and not a["off"]]
    assert any(a["flush"] for _, a in calls)
    assert any(a["flush"] and a["n"] == 0 and sh["flush_inputs"] > 0 for sh, a in calls)
    assert any(0 < a["n"] < sh["H"] - 1 for sh, a in calls)                     # shorter than the history
    assert any(0 < sh["L"] * a["n"] < sh["Nd"] - 1 for sh, a in calls)          # the sliding rule
    assert any(a["n"] > 4096 for _, a in calls)                                 # an interior tile
    # ... and the single operators in turn with it on the same handles
    assert any({a["fused"] for a in _steps(ops)} == {True, False} for _, ops in fused)
    assert any(a["off"] for sh, ops in fused for a in _steps(ops) if a["fused"])


def test_chain_draws_reach_every_trait_off_the_fused_kernel():
    shapes = [sh for sh, _ in CHAINS]
    assert {sh["taps_kind"] for sh in shapes} == set(F.TAPS_KINDS)
    assert any(sh["L"] in (1, 9, 16) for sh in shapes) and any(sh["M"] in (12, 16) for sh in shapes)
    assert any(sh["uvar"] == 1 for sh in shapes) and any(sh["dvar"] == 2 for sh in shapes)
    assert any(not F.int16_range(sh["cu"]) for sh in shapes) and any(not F.int16_range(sh["cd"]) for sh in shapes)
    assert any(sh["Nd"] > F.MAX_DECIM_TAPS for sh in shapes)
    assert any(sh["flush_inputs"] < sh["H"] for sh in shapes if F.eligible(sh))  # a zero tail: a shorter flush
    for name in ("set_left_shift", "reset_up", "reset_decim", "copy"):
        assert any(op[0] == name for _, ops in CHAINS for op in ops), name


def test_bank_draws_reach_both_paths():
    one = [sh for sh in BANKS
           if F.bank_eligible(sh) and any(n > 0 or (f and sh["flush_inputs"]) for n, f in sh["calls"])]
    assert len(one) >= 3 and any(sh["rows"] == 65 for sh in one), [sh["rows"] for sh in one]
    assert {sh["rows"] for sh in BANKS} == {1, 2, 5, 65}
    assert any(F.eligible(sh) and not sh["in_stride16"] for sh in BANKS)
    assert any(F.eligible(sh) and not sh["out_stride16"] for sh in BANKS)
    assert any(f for sh in one for _, f in sh["calls"])
