"""srcdsp_corr_step_batched: C correlators stepped in one call, on one input per
channel or on one shared input.  Every comparison is bit-exact against one
O["fma"].corr(N, S) per channel stepped with the same chunks
(correlators.h:209-303): found, corrIndex, bitSamples and the energy / corr /
coeffs_energy / coeff_scaling status fields, after every call.  The
process-wide counters prove which path (bank kernel / per-channel loop) served
a call.

Signal (the recipe of test_correlator_vs_oracle): noise uniform in +-125 and
x[off + m] += 2 p[m] for a QPSK pattern p of amplitude 500.  The oracle detects
such a burst at the pattern's last sample, corrIndex = off + N - 1, so the
scan's `best` (the sample after the peak) is off + N.  Each test asserts that
the oracle alone produced the positions the signal was built for, so a signal
that stops detecting cannot make a test pass empty."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096            # outputs per workgroup of the scan
N_CASE1 = 3 * TILE + 500
FIELDS = ("energy", "corr", "coeffs_energy", "coeff_scaling")
FREQS = [0.0, 0.1, -0.37, 0.5, 0.73, -0.2, 0.3, -0.45]  # as test_gpu_ddc_bank.py


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def pattern(N, seed, amplitude=None):
    from srcdsp_amd.design import qpsk_pattern
    return qpsk_pattern(N, (500 if N <= 2048 else 200) if amplitude is None else amplitude, seed=seed)


def signal(n, seed, bursts, S_=1):
    """Noise +-125 with x[off + m S] += 2 p[m] for every (off, p) of `bursts`."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-125, 126, size=(n, 2)).astype(np.int32)
    for off, p in bursts:
        for m in range(len(p)):
            if 0 <= off + m * S_ < n:
                x[off + m * S_] += 2 * p[m]
    return np.clip(x, -32768, 32767).astype(np.int16)


def case1_signal(N, C):
    """Case 1's channels: `best` of each channel's first burst on tile residues
    0, 1, 2, 4095 and 17 (in the second tile), one channel with no burst, the
    others with two bursts; every channel its own pattern and noise.  Returns
    (patterns, x [C, n, 2], the designed `best` of each channel's first burst
    or None)."""
    first = {1: [TILE], 3: [TILE + 1, TILE - 1, None],
             8: [TILE, TILE + 1, TILE + 2, TILE - 1, TILE + 17, None, 2 * TILE, 2 * TILE - 1]}[C]
    ps = [pattern(N, 100 * N + c) for c in range(C)]
    xs = []
    for c in range(C):
        b = [] if first[c] is None else [(first[c] - N, ps[c])]
        if c >= 6:
            b.append((first[c] + 1500, ps[c]))
        xs.append(signal(N_CASE1, 7 * N + c, b))
    return ps, np.stack(xs), first


def make(S, O, ps, N, S_=1):
    cors, refs = [], []
    for p in ps:
        g, r = S.FixedPatternCorrelator(N, S_), O["fma"].corr(N, S_)
        g.setPattern(p)
        r.set_pattern(p)
        cors.append(g)
        refs.append(r)
    return cors, refs


def check(g, r, got, want, tag):
    assert (got[0], got[0] and got[1]) == (want[0], want[0] and want[1]), (tag, got, want)
    assert np.array_equal(g.getRefBitSamples(), r.bit_samples()), tag
    st, sr = g.getStatus(), r.status()
    assert all(st[k] == sr[k] for k in FIELDS), (tag, st, sr)


def run_stepping(S, cors, refs, x, caps=()):
    """Step on after each detection, as a receiver does: channel c continues at
    its own position (corrIndex + 2 past the call's start after a detection).
    The channels are then no longer in lock-step, so every round is one
    batched call on the channels' common remaining prefix (the shortest
    remainder, or caps[round] if shorter), each channel's row starting at its
    own position; a channel that has consumed its input leaves the bank.
    Returns (events[c] = [(call start, corrIndex)], calls)."""
    import torch
    ch, n = x.shape[0], x.shape[1]
    xd = dev(x)
    pos, events, calls = [0] * ch, [[] for _ in range(ch)], 0
    while True:
        act = [c for c in range(ch) if pos[c] < n]
        if not act:
            return events, calls
        m = min(n - pos[c] for c in act)
        if calls < len(caps):
            m = min(m, caps[calls])
        rows = torch.stack([xd[c, pos[c]:pos[c] + m] for c in act])
        got = S.corr_step_batched([cors[c] for c in act], rows)
        for k, c in enumerate(act):
            want = refs[c].step(x[c, pos[c]:pos[c] + m])
            check(cors[c], refs[c], got[k], want, (calls, c, pos[c], m))
            if want[0]:
                events[c].append((pos[c], want[1]))
            pos[c] += want[1] + 2 if want[0] else m
        calls += 1


def run_fixed(call, cors, refs, rows, chunks):
    """Every channel takes every chunk whole (samples after a detection inside
    a chunk are dropped, as the reference's break drops them).  `call(off, m)`
    runs the batched step on samples off .. off + m of every channel; rows[c]
    is channel c's host signal.  Returns events[c] = [(off, corrIndex)]."""
    events, off = [[] for _ in cors], 0
    for m in chunks:
        got = call(off, m)
        for c in range(len(cors)):
            want = refs[c].step(rows[c][off:off + m])
            check(cors[c], refs[c], got[c], want, (off, m, c))
            if want[0]:
                events[c].append((off, want[1]))
        off += m
    return events


def capi_call(S, cors, base, first, in_stride, stream=None):
    """srcdsp_corr_step_batched through the C ABI: channel c reads samples
    first + c * in_stride .. of the int16 [*, 2] device tensor `base`."""
    import torch
    from srcdsp_amd import _capi as A
    ch = len(cors)
    hs = (C.c_void_p * ch)(*[g._h.value for g in cors])

    def call(off, m):
        found, idx = (C.c_int * ch)(), (C.c_int * ch)(*([-7] * ch))
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = A.lib().srcdsp_corr_step_batched(hs, ch, C.c_void_p(base.data_ptr() + 4 * (first + off)), in_stride, m,
                                              found, idx, C.c_void_p(st))
        assert rc == 0, A.lib().srcdsp_last_error()
        return [(bool(found[c]), idx[c]) for c in range(ch)]
    return call


# ------------------------------------- 1. independent inputs, bank kernel
@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("C_", [1, 3, 8])
def test_independent_inputs_bank_kernel(S, O, C_, N):
    ps, x, first = case1_signal(N, C_)
    cors, refs = make(S, O, ps, N)
    b0, l0 = S.corr_batched_stats()
    events, calls = run_stepping(S, cors, refs, x)
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (calls, 0)
    # the oracle found every first burst where it was placed (round 1 starts
    # every channel at 0, so the corrIndex + 1 there is the scan's `best`)
    for c in range(C_):
        if first[c] is None:
            assert events[c] == [], c
        else:
            assert events[c][0] == (0, first[c] - 1), (c, events[c])
            assert len(events[c]) >= (2 if c >= 6 else 1), (c, events[c])
    if C_ == 8:
        res = {(e[0][1] + 1) % TILE for e in events if e}
        assert {0, 1, 2, TILE - 1, 17} <= res, res


# ---------------------------------------------------- 2. call boundaries
@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("L", [4999, 5000, 5001, 5002])
def test_call_boundaries_use_the_carried_registers(S, O, L, N):
    """One burst ending at sample 5000 (best = 5001) and a first call of L
    samples: the hit lands at corrIndex 1, 0 or -1 of the second call (the
    peak test then reads the registers carried from the first), or inside the
    first; then a call of 5 samples (shorter than a lane's 16 outputs) and one
    of 100 (shorter than the history at N = 1024)."""
    C_, n = 3, 5000 + TILE + 300
    ps = [pattern(N, 200 * N + c) for c in range(C_)]
    x = np.stack([signal(n, 11 * N + c, [(5001 - N, ps[c])]) for c in range(C_)])
    cors, refs = make(S, O, ps, N)
    b0, l0 = S.corr_batched_stats()
    events, calls = run_stepping(S, cors, refs, x, caps=(L, 5, 100))
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (calls, 0)
    for c in range(C_):
        assert events[c] and events[c][0] == ((0, 5000) if L == 5002 else (L, 5000 - L)), (c, events[c])


# -------------------------------------------- 3. N not a multiple of 16
@pytest.mark.parametrize("N", [1, 17, 33, 100, 1000])
def test_tap_counts_off_the_multiple_of_16(S, O, N):
    C_, n = 3, TILE + 1500
    ps = [pattern(N, 300 * N + c) for c in range(C_)]
    want_best = [TILE, TILE + 1, TILE - 1]
    x = np.stack([signal(n, 13 * N + c, [(want_best[c] - N, ps[c])]) for c in range(C_)])
    cors, refs = make(S, O, ps, N)
    b0, l0 = S.corr_batched_stats()
    events, calls = run_stepping(S, cors, refs, x, caps=(5000,))
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (calls, 0)
    # N = 1 and N = 17 stay under the threshold for this signal in the oracle
    # too (as in test_correlator_vs_oracle's list): registers at every step
    if N not in (1, 17):
        for c in range(C_):
            assert events[c] and events[c][0] == (0, want_best[c] - 1), (c, events[c])


# ------------------------------------------------------ 4. shared input
def test_shared_input_each_pattern_finds_its_own(S, O):
    N, n = 64, N_CASE1
    ps = [pattern(N, 40 + c) for c in range(4)]
    ps[3] = 2 * ps[3]  # every component doubled: coeff_scaling one up
    x = signal(n, 4, [(TILE + 1 - N, ps[0])])
    x[2 * TILE + 700:2 * TILE + 700 + N] += ps[3].astype(np.int16)  # = 2 x the pattern of amplitude 500
    cors, refs = make(S, O, ps, N)
    cs = [g.getStatus()["coeff_scaling"] for g in cors]
    assert cs[3] != cs[0] and cs[0] == cs[1] == cs[2], cs
    xd = dev(x)
    b0, l0 = S.corr_batched_stats()
    chunks = [5000, TILE + 36, n - 5000 - TILE - 36]
    events = run_fixed(lambda off, m: S.corr_step_batched(cors, xd[off:off + m]), cors, refs, [x] * 4, chunks)
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (len(chunks), 0)
    assert events[0] == [(0, TILE)], events
    assert events[3] == [(5000, 2 * TILE + 700 + N - 1 - 5000)], events
    assert events[1] == [] and events[2] == [], events


# ------------------------------------------------------ 5. row alignment
@pytest.mark.parametrize("first", [0, 1], ids=["aligned_base", "base_off_by_one_sample"])
def test_rows_of_differing_alignment(S, O, first):
    """in_stride = n + 1 through the C ABI: consecutive rows sit 4 bytes off
    each other's 16-byte alignment (row 4 shares row 0's), from an aligned
    base and from a device view one sample off a 16-byte boundary."""
    import torch
    N, C_, n = 64, 5, 2 * TILE + 1024
    ps = [pattern(N, 50 + c) for c in range(C_)]
    bests = [TILE, TILE + 1, TILE + 2, TILE - 1, TILE + 17]
    rows = [signal(n, 60 + c + first, [(bests[c] - N, ps[c]), (TILE + 3000 + c, ps[c])]) for c in range(C_)]
    flat = np.zeros((first + C_ * (n + 1), 2), np.int16)
    for c in range(C_):
        flat[first + c * (n + 1):first + c * (n + 1) + n] = rows[c]
    base = dev(flat)
    assert base.data_ptr() % 16 == 0
    cors, refs = make(S, O, ps, N)
    b0, l0 = S.corr_batched_stats()
    chunks = [6000, n - 6000]
    events = run_fixed(capi_call(S, cors, base, first, n + 1), cors, refs, rows, chunks)
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (2, 0)
    for c in range(C_):
        assert events[c][0] == (0, bests[c] - 1) and len(events[c]) == 2, (c, events[c])
    torch.cuda.synchronize()


# --------------------------------------------------------- 6. 65 channels
def test_past_the_batch_limit(S, O):
    """65 channels: two launches of the bank kernel (64 + 1) inside one call,
    counted as one call; a burst in every eighth channel, the 65th included."""
    N, C_, n = 64, 65, TILE + 36 + 300
    ps = [pattern(N, 70 + c % 3) for c in range(C_)]
    rows = [signal(n, 500 + c, [(TILE + 20 - N, ps[c])] if c % 8 == 0 else []) for c in range(C_)]
    cors, refs = make(S, O, ps, N)
    xd = dev(np.stack(rows))
    b0, l0 = S.corr_batched_stats()
    chunks = [TILE + 36, 300]
    events = run_fixed(lambda off, m: S.corr_step_batched(cors, xd[:, off:off + m].contiguous()), cors, refs, rows,
                       chunks)
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (2, 0)
    for c in range(C_):
        assert events[c][:1] == ([(0, TILE + 19)] if c % 8 == 0 else []), (c, events[c])


def test_lead_scratch_grows_and_is_reused(S, O):
    """The bank's scratch lives on hs[0] and only grows: one lead through calls
    of 2, 5 and 2 channels (kept, regrown, reused at the larger capacity), each
    call against single-channel steps on clones; a burst in the last channel of
    every call, so its bitSamples row is copied back."""
    import copy
    N, n = 64, 2048
    ps = [pattern(N, 40 + c) for c in range(5)]
    cors, _ = make(S, O, ps, N)
    b0, l0 = S.corr_batched_stats()
    for call, ch in enumerate((2, 5, 2)):
        x = np.stack([signal(n, 900 + 10 * call + c, [(700 + call, ps[c])] if c == ch - 1 else []) for c in range(ch)])
        twins = [copy.copy(g) for g in cors[:ch]]
        xd = dev(x)
        got = S.corr_step_batched(cors[:ch], xd)
        assert [f for f, _ in got] == [c == ch - 1 for c in range(ch)], (call, got)
        assert got[ch - 1][1] == 700 + call + N - 1, (call, got)
        for c in range(ch):
            want = twins[c].step(xd[c])
            assert (got[c][0], got[c][0] and got[c][1]) == (want[0], want[0] and want[1]), (call, c, got[c], want)
            assert cors[c].getStatus() == twins[c].getStatus(), (call, c)
            assert np.array_equal(cors[c].getRefBitSamples(), twins[c].getRefBitSamples()), (call, c)
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (3, 0)


# ------------------------------------------------------------ 7. hand-over
def test_state_equals_single_channel_api_and_hands_over(S, O):
    import copy
    N, C_ = 64, 3
    ps, x, _ = case1_signal(N, C_)
    cors, refs = make(S, O, ps, N)
    twins, _ = make(S, O, ps, N)
    xd = dev(x)
    chunks = [5000, TILE + 36, N_CASE1 - 5000 - TILE - 36]
    rows = [x[c] for c in range(C_)]
    events = run_fixed(lambda off, m: S.corr_step_batched(cors, xd[:, off:off + m].contiguous()), cors, refs, rows,
                       chunks)
    assert sum(len(e) for e in events) >= 2
    extra = signal(3000, 99, [(1000, ps[0])])
    off = 0
    for m in chunks:
        for c in range(C_):
            twins[c].step(xd[c, off:off + m])
        off += m
    for c in range(C_):
        st, s1 = cors[c].getStatus(), twins[c].getStatus()
        assert st == s1, c
        assert np.array_equal(cors[c].getRefBitSamples(), twins[c].getRefBitSamples()), c
        clone = copy.copy(cors[c])
        want = refs[c].step(extra)
        # one further single-channel step on the batched handle and on its clone
        for g in (cors[c], clone):
            check(g, refs[c], g.step(dev(extra)), want, c)


def test_batched_then_single_channel_on_another_stream(S, O):
    """A batched call on a side stream, then a single-channel step on the
    default stream on one of its handles, with no host synchronise between."""
    import torch
    N, C_, n = 64, 3, 1 << 16
    ps = [pattern(N, 80 + c) for c in range(C_)]
    rows = [signal(2 * n, 90 + c, [(n + 3000 + c, ps[c])]) for c in range(C_)]
    cors, refs = make(S, O, ps, N)
    xd = dev(np.stack(rows))
    first = xd[:, :n].contiguous()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = S.corr_step_batched(cors, first)
    g1 = cors[1].step(xd[1, n:])  # default stream
    torch.cuda.synchronize()
    for c in (0, 2):
        check(cors[c], refs[c], got[c], refs[c].step(rows[c][:n]), c)
    assert got[1][0] is False and refs[1].step(rows[1][:n])[0] is False
    w1 = refs[1].step(rows[1][n:])
    assert w1 == (True, 3000 + 1 + N - 1)
    check(cors[1], refs[1], g1, w1, "second step")


# ------------------------------------------------------ 8. fallback shapes
@pytest.mark.parametrize("N,S_", [(32, 4), (64, 2), (8200, 1)])
def test_fallback_shapes_take_the_loop_and_stay_exact(S, O, N, S_):
    C_, n = 2, 20000
    ps = [pattern(N, 90 * N + c) for c in range(C_)]
    x = np.stack([signal(n, 17 * N + c, [(9000 + 100 * c, ps[c])], S_) for c in range(C_)])
    cors, refs = make(S, O, ps, N, S_)
    b0, l0 = S.corr_batched_stats()
    events, calls = run_stepping(S, cors, refs, x, caps=(12000,))
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (0, calls)
    assert sum(len(e) for e in events) >= C_, events


# ------------------------------------------------------------- 9. errors
def test_errors_change_no_state(S, O):
    import torch
    from srcdsp_amd import _capi as A
    N, n = 64, 6000
    ps = [pattern(N, 20 + c) for c in range(2)]
    x = np.stack([signal(n, 40 + c, [(3000, ps[c])]) for c in range(2)])
    cors, refs = make(S, O, ps, N)
    xd = dev(x)
    got = S.corr_step_batched(cors, xd)  # some state to keep (a detection: bitSamples set)
    assert [g[0] for g in got] == [True, True]
    other_n, other_s = S.FixedPatternCorrelator(32, 1), S.FixedPatternCorrelator(64, 2)
    other_n.setPattern(pattern(32, 1))
    other_s.setPattern(pattern(64, 2))

    def snapshot():
        return [(g.getStatus(), g.getRefBitSamples().copy()) for g in cors + [other_n, other_s]]

    before, stats = snapshot(), S.corr_batched_stats()
    for bad in ([cors[0], other_n], [cors[0], other_s], [cors[0], cors[0]]):
        with pytest.raises(S.SrcdspError) as e:
            S.corr_step_batched(bad, xd)
        assert e.value.code == A.ERR_ARG
    # n beyond INT_MAX: the count alone (refused before any sample is read)
    hs = (C.c_void_p * 2)(*[g._h.value for g in cors])
    found, idx = (C.c_int * 2)(), (C.c_int * 2)()
    rc = A.lib().srcdsp_corr_step_batched(hs, 2, C.c_void_p(xd.data_ptr()), n, (1 << 31), found, idx, None)
    assert rc == A.ERR_SIZE
    # n == 0: OK, nothing found, nothing changed
    found[0] = found[1] = 5
    assert A.lib().srcdsp_corr_step_batched(hs, 2, None, 0, 0, found, idx, None) == 0
    assert list(found) == [0, 0]
    with pytest.raises(ValueError):
        S.corr_step_batched(cors, xd[:1])            # one row, two correlators
    with pytest.raises(ValueError):
        S.corr_step_batched(cors, xd[:, :, 0])       # not [.., 2]
    with pytest.raises(ValueError):
        S.corr_step_batched([], xd)
    with pytest.raises(TypeError):
        S.corr_step_batched(cors, x)                 # host input
    assert S.corr_batched_stats() == stats
    after = snapshot()
    for (s0, b0), (s1, b1) in zip(before, after):
        assert s0 == s1 and np.array_equal(b0, b1)
    torch.cuda.synchronize()


# ------------------------------------------------- 10. exact-sqrt build
def test_always_exact_build_gives_the_same_detections(S, O, tmp_path):
    """Case 1's N = 64 signal through the batched call of the always-exact
    library, in a child process that holds only that library
    (tests/corr_bank_exact_child.py), against the product library here."""
    import json
    import subprocess
    import sys
    exact = os.path.join(ROOT, "tests", "_build", "libsrcdsp_hip_corr_exact.so")
    assert os.path.exists(exact), f"{exact} not built: run python -c 'import __graft_entry__ as g; g.build()'"
    out = str(tmp_path / "bank_exact.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "corr_bank_exact_child.py"), exact, out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["product_mapped"] is False and res["build_flags"] == 1
    assert res["stats"] == [res["calls"], 0]
    ps, x, first = case1_signal(64, 8)
    cors, refs = make(S, O, ps, 64)
    events, calls = run_stepping(S, cors, refs, x)
    assert calls == res["calls"]
    assert [[list(e) for e in ev] for ev in events] == res["events"]
    assert sum(len(e) for e in events) >= 7


# ------------------------------------- 11. channelised search, end to end
def test_channelised_search_end_to_end(S, O):
    """One wideband input -> mixdecim_step_batched (8 LOs, 63 taps, M = 4) ->
    corr_step_batched (N = 64), device-resident throughout, against
    om -> od -> oc per channel.  The input is noise plus the pattern held 4
    samples per symbol and rotated by channel 1's LO conjugate (the oracle
    mixer at -f), so that it lands in that channel after mixing.  Pattern
    amplitude 700: sqrt(coeffs_energy) = 7920 sits high in its octave, which
    leaves the peak test the margin the channel filter's intersymbol
    interference takes (at amplitude 500 the ratio of a clean match is 2.76
    against the threshold 2.7).  Which channel fires is the oracle's say."""
    import torch
    from srcdsp_amd.design import hamming_sinc, q14
    n, N, C_, M = 65536, 64, 8, 4
    cq = q14(hamming_sinc(63))
    p = pattern(N, 11, amplitude=700)
    base = np.zeros((n, 2), np.int16)
    for off in (30003, 50003):
        base[off:off + 4 * N] = np.repeat(2 * p, 4, axis=0)
    conj = O["strict"].mixer(4096)
    conj.reset(-FREQS[1])
    rng = np.random.default_rng(5)
    x = np.clip(conj.step(base).astype(np.int32) + rng.integers(-125, 126, size=(n, 2)), -32768, 32767)
    x = x.astype(np.int16)
    ci16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")
    ms, ds, cors, chain = [], [], [], []
    for c in range(C_):
        m = S.Mixer(4096)
        m.reset(FREQS[c])
        ms.append(m)
        ds.append(S.FilterDnsamplingFir(cq, M, *ci16))
        g = S.FixedPatternCorrelator(N, 1)
        g.setPattern(p)
        cors.append(g)
        om, od, oc = O["strict"].mixer(4096), O["strict"].decim(1, M, cq), O["fma"].corr(N, 1)
        om.reset(FREQS[c])
        oc.set_pattern(p)
        chain.append((om, od, oc))
    xd = dev(x)
    events = 0
    b0, l0 = S.corr_batched_stats()
    chunks = [40000, n - 40000]
    off = 0
    for m_ in chunks:
        y = torch.empty((C_, m_ // M, 2), dtype=torch.int16, device="cuda")
        S.mixdecim_step_batched(ms, ds, xd[off:off + m_], y)
        got = S.corr_step_batched(cors, y)
        for c, (om, od, oc) in enumerate(chain):
            want = oc.step(od.step(om.step(x[off:off + m_])))
            check(cors[c], oc, got[c], want, (off, c))
            events += want[0]
        off += m_
    b1, l1 = S.corr_batched_stats()
    assert (b1 - b0, l1 - l0) == (len(chunks), 0)
    assert events >= 1
