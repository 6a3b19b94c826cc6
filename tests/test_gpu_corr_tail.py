"""The end of a correlator step (csrc/corr_tail.h: registers with their
reach-back into the previous call, the new history, bitSamples) behind every
scan path of the single-channel calls, behind prime() and behind the host,
trace and clone entry points.  Every comparison after every call is bit-exact
against O["fma"].corr(N, S) (correlators.h:209-303): found, corrIndex,
bitSamples and the energy / corr / coeffs_energy / coeff_scaling status.

Signal: n = N S + 700 samples of noise uniform in +-125 from default_rng(N),
x[300 + m S] += 2 p[m] for qpsk_pattern(N, 500 (200 past 2048 taps), seed=N).
The oracle detects the burst at its last sample, corrIndex P = 300 + (N - 1) S,
when it processes sample P + 1.  Every test requires of the oracle alone
exactly that one detection, so a signal that stops detecting cannot make a
test pass empty."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("energy", "corr", "coeffs_energy", "coeff_scaling")
# (N, S): the fused scan, the fused scan off a multiple of 16 taps, corr_eval,
# corr_eval_dot2, the generic kernel past 8192 taps
SHAPES = [(64, 1), (33, 1), (32, 4), (64, 2), (8200, 1)]


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()  # a copy: the shared signal is read-only


@functools.lru_cache(maxsize=None)
def case(N, S_):
    """(pattern, signal, P) of a shape; shared by the tests, never written to."""
    from srcdsp_amd.design import qpsk_pattern
    p = qpsk_pattern(N, 500 if N <= 2048 else 200, seed=N)
    n = N * S_ + 700
    x = np.random.default_rng(N).integers(-125, 126, size=(n, 2)).astype(np.int32)
    for m in range(N):
        x[300 + m * S_] += 2 * p[m]
    x = np.clip(x, -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return p, x, 300 + (N - 1) * S_


def plans(P, n):
    """Call lengths; a call starts corrIndex + 2 past the previous one's start
    after a detection, else where that one ended; the last length repeats."""
    return {"whole": [n],
            "hit_at_0_of_1": [P + 1, 1, 1, 1, n],  # the hit is the first sample of a 1-sample call
            "hit_at_1_of_2": [P, 2, 2, n],
            "hit_at_2_of_3": [P - 1, 3, 3, n],
            "calls_of_1": [P - 3] + [1] * 8 + [n],
            "calls_of_2": [P - 4] + [2] * 5 + [n]}


PLAN_IDS = sorted(plans(0, 0))


def make(S, O, N, S_, p):
    g, r = S.FixedPatternCorrelator(N, S_), O["fma"].corr(N, S_)
    g.setPattern(p)
    r.set_pattern(p)
    return g, r


def check_status(g, r, tag):
    st, sr = g.getStatus(), r.status()
    assert all(st[k] == sr[k] for k in FIELDS), (tag, st, sr)


def check(g, r, got, want, tag):
    assert (got[0], got[0] and got[1]) == (want[0], want[0] and want[1]), (tag, got, want)
    assert np.array_equal(g.getRefBitSamples(), r.bit_samples()), tag
    check_status(g, r, tag)


def run_plan(x, plan, r, call, first=0):
    """Walks `plan` over x[first:]: call(pos, chunk) steps the correlator under
    test and checks it against the oracle r, which has just taken the same
    chunk with result `want`.  Returns the oracle's detections (global corrIndex)."""
    pos, k, events = first, 0, []
    while pos < len(x):
        xs = x[pos:pos + plan[min(k, len(plan) - 1)]]
        want = r.step(xs)
        call(pos, xs, want)
        if want[0]:
            events.append(pos + want[1])
        pos += want[1] + 2 if want[0] else len(xs)
        k += 1
    return events


# ------------------------- short calls and reach-back on every scan path
@pytest.mark.parametrize("plan", PLAN_IDS)
@pytest.mark.parametrize("N,S_", SHAPES)
def test_short_calls_reach_back_on_every_scan_path(S, O, N, S_, plan):
    """A hit at call index 0, 1 and 2, no-hit calls of 1, 2 and 3 samples (one
    or two registers come from the previous call) and histories taken mostly
    from the old history."""
    p, x, P = case(N, S_)
    g, r = make(S, O, N, S_, p)
    xd = dev(x)

    def call(pos, xs, want):
        check(g, r, g.step(xd[pos:pos + len(xs)]), want, (plan, pos, len(xs)))

    assert run_plan(x, plans(P, len(x))[plan], r, call) == [P]


# ---------------------------------------- prime() against the oracle's
@pytest.mark.parametrize("halo", [1, 2, 3, "NS+2"])
@pytest.mark.parametrize("N,S_", [(64, 1), (32, 4)])
def test_prime_equals_the_oracles_prime(S, O, N, S_, halo):
    p, x, P = case(N, S_)
    h = N * S_ + 2 if halo == "NS+2" else halo
    g, r = make(S, O, N, S_, p)
    g.prime(dev(x[200 - h:200]))
    r.prime(x[200 - h:200])
    check_status(g, r, ("prime", h))
    xd = dev(x)

    def call(pos, xs, want):
        check(g, r, g.step(xd[pos:pos + len(xs)]), want, (h, pos, len(xs)))

    assert run_plan(x, [len(x)], r, call, first=200) == [P]


# ------------------------------ host, trace and clone entry points
@pytest.mark.parametrize("entry", ["step_host", "step_trace", "step_host_trace"])
@pytest.mark.parametrize("N,S_", [(64, 1), (32, 4)])
def test_host_trace_and_clone_entry_points(S, O, N, S_, entry):
    """Plan [P, 2, 2, n] through step_host / step_trace (device and host
    input); every call runs on a copy.copy of the handle the call before left.
    The trace arrays equal oracle.registers over the processed samples, from
    an oracle brought to the call's start by the same chunks."""
    p, x, P = case(N, S_)
    g, r = make(S, O, N, S_, p)
    cur, done = [g], []

    def call(pos, xs, want):
        h = copy.copy(cur[0])
        if entry == "step_host":
            got = h.step(xs)
        else:
            found, idx, c, e = h.step_trace(dev(xs) if entry == "step_trace" else xs)
            got = (found, idx)
            t = O["fma"].corr(N, S_)
            t.set_pattern(p)
            for chunk in done:
                t.step(chunk)
            k = want[1] + 2 if want[0] else len(xs)  # the processed samples
            wc, we = t.registers(xs[:k])
            assert len(c) == k and np.array_equal(c, wc) and np.array_equal(e, we), (pos, k)
        check(h, r, got, want, (entry, pos, len(xs)))
        cur[0] = h
        done.append(xs)

    assert run_plan(x, plans(P, len(x))["hit_at_1_of_2"], r, call) == [P]
