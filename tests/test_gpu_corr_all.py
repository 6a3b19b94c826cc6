"""srcdsp_corr_step_all: every detection of a stream in one call.  Every
comparison is bit-exact against the oracle loop (corr_all_model.step_all over
O["fma"].corr: step() called again on the remainder after each detection,
correlators.h:209-303): indices, bitSamples rows, consumed and the energy /
corr status fields after every call, then one ordinary step on fresh samples,
which proves the history.  The process-wide counters prove which path (the
kernels / the loop of srcdsp_corr_step) served a call.

The rows come from corr_all_model.cases(); tests/test_corr_all_model.py pins on
the CPU what the oracle loop finds in them (the planted bursts; on the
back-to-back rows not the points where the undisturbed test fires), so no test
here can pass on "nothing found"."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import corr_all_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("energy", "corr", "coeffs_energy", "coeff_scaling")
CASES = M.cases()


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def pair(S, O, N, p, S_=1):
    g, r = S.FixedPatternCorrelator(N, S_), O["fma"].corr(N, S_)
    g.setPattern(p)
    r.set_pattern(p)
    return g, r


def same_state(g, r, tag):
    st, sr = g.getStatus(), r.status()
    assert all(st[k] == sr[k] for k in FIELDS), (tag, st, sr)
    assert np.array_equal(g.getRefBitSamples(), r.bit_samples()), tag


def follow(g, r, p, tag):
    """One ordinary step on fresh samples with a burst: the history."""
    extra = M.signal(1500, 4242, [(600, p)])
    want = r.step(extra)
    assert want == (True, 600 + len(p) - 1), (tag, want)
    assert g.step(dev(extra)) == want, tag
    same_state(g, r, tag)


def run_case(S, O, case, view=lambda t: t):
    """The case's calls on the GPU and through the oracle loop in lock-step;
    returns the GPU's calls."""
    N, p, x, chunks, mh = case
    g, r = pair(S, O, N, p)
    xd = view(dev(x))
    pos = [0]

    def gpu(xs, m):  # run_calls slices the host row; the device row is sliced alike
        out = g.stepAll(xd[pos[0]:pos[0] + len(xs)], m)
        pos[0] += out[2]
        return out

    def ref(xs, m):
        out = M.step_all(r, xs, m)
        states.append(r.status())
        return out

    states, got_states = [], []
    want = M.run_calls(ref, x, chunks, mh)
    k0, l0 = S.corr_all_stats()
    got = M.run_calls(lambda xs, m: (gpu(xs, m), got_states.append(g.getStatus()))[0], x, chunks, mh)
    k1, l1 = S.corr_all_stats()
    assert (k1 - k0, l1 - l0) == (len(want), 0)
    M.same_calls(got, want)
    for a, b in zip(got_states, states):
        assert all(a[k] == b[k] for k in FIELDS), (a, b)
    same_state(g, r, "end")
    follow(g, r, p, "follow")
    return got


pytestmark = pytest.mark.gpu


# --------------------------------------------------- 1. the single-row cases
@pytest.mark.parametrize("name", sorted(CASES))
def test_single_row_cases(S, O, name):
    """Sparse bursts with a detection in outputs 0, 1, 15, 16, 4095 of a tile
    and 0, 1 of the next; back-to-back bursts with gaps 0, 1, 2 (N = 32, 33,
    64); a patch over a tile boundary; a patch past the end of the call; a
    detection at the call's first sample (index -1); n < N; max_hits reached,
    then the remainder."""
    got = run_case(S, O, CASES[name])
    assert sum(len(c[1]) for c in got) >= 1


def test_max_hits_then_remainder_equal_one_call(S, O):
    N, p, x, _, _ = CASES["max_hits_exact"]
    g, r = pair(S, O, N, p)
    whole = g.stepAll(dev(x), 1000)
    assert len(whole[0]) == 7 and whole[2] == len(x)
    parts = run_case(S, O, CASES["max_hits_exact"])
    assert [len(c[1]) for c in parts] == [7, 0]
    assert parts[0][1] == whole[0].tolist() and np.array_equal(parts[0][2], whole[1])


def test_unaligned_input_view(S, O):
    """The row one sample off a 16-byte boundary."""
    case = CASES["tile_%d" % (M.TILE + 1)]

    def view(t):
        import torch
        buf = torch.zeros((len(t) + 1, 2), dtype=torch.int16, device="cuda")
        buf[1:] = t
        assert buf.data_ptr() % 16 == 0 and buf[1:].data_ptr() % 16 == 4
        return buf[1:]

    run_case(S, O, case, view)


def test_host_input_is_staged(S, O):
    N, p, x, _, _ = CASES["b2b_32_1"]
    g, r = pair(S, O, N, p)
    got, want = g.stepAll(x, 64), M.step_all(r, x, 64)
    assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]) and got[2] == want[2]
    same_state(g, r, "host")
    follow(g, r, p, "host")


# ------------------------------------------------------------- 2. batched
def _batched(S, O, N, ps, rows, shared=None, mh=64):
    gs, rs = zip(*[pair(S, O, N, p) for p in ps])
    xd = dev(shared if shared is not None else np.stack(rows))
    k0, l0 = S.corr_all_stats()
    got = S.corr_step_all_batched(list(gs), xd, mh)
    k1, l1 = S.corr_all_stats()
    assert (k1 - k0, l1 - l0) == (1, 0)
    hits = []
    for c, (g, r) in enumerate(zip(gs, rs)):
        want = M.step_all(r, shared if shared is not None else rows[c], mh)
        assert got[c][0].tolist() == want[0].tolist() and got[c][2] == want[2], (c, got[c][0], want[0])
        assert np.array_equal(got[c][1], want[1]), c
        same_state(g, r, c)
        hits.append(len(want[0]))
    for c in (0, len(ps) - 1):
        follow(gs[c], rs[c], ps[c], c)
    return hits


def test_batched_rows_on_every_tile_residue(S, O):
    names = ["tile_%d" % q for q in M.TILE_Q]
    hits = _batched(S, O, 64, [CASES[k][1] for k in names], [CASES[k][2] for k in names])
    assert hits == [3] * 7


def test_shared_input_each_pattern_finds_its_own(S, O):
    N = 64
    ps = [M.pattern(N, 40 + c) for c in range(3)]
    x = M.signal(M.N_TILES, 44, [(1000, ps[0]), (1064, ps[0]), (M.TILE - 30, ps[1]), (9000, ps[0]), (9500, ps[1])],
                 gain=4)
    hits = _batched(S, O, N, ps, None, shared=x)
    assert hits[0] >= 2 and hits[1] == 2 and hits[2] == 0, hits


def test_past_the_batch_limit(S, O):
    """65 channels: two launches of each kernel (64 + 1) inside one call."""
    N, C_, n = 32, 65, M.TILE + 300
    ps = [M.pattern(N, 70 + c % 3) for c in range(C_)]
    rows = [M.signal(n, 500 + c, [(M.TILE - 40 + c, ps[c]), (M.TILE - 8 + c, ps[c])] if c % 8 == 0 else [], gain=8,
                     noise=200) for c in range(C_)]
    hits = _batched(S, O, N, ps, rows)
    assert all((h >= 1) == (c % 8 == 0) for c, h in enumerate(hits)), hits


# ------------------------------------------------------- 3. the loop path
def test_stride_4_takes_the_loop_and_stays_exact(S, O):
    N, S_ = 32, 4
    p = M.pattern(N, 91)
    rng = np.random.default_rng(92)
    x = rng.integers(-125, 126, size=(6000, 2)).astype(np.int32)
    for off in (700, 2500, 4000):
        for m in range(N):
            x[off + m * S_] += 2 * p[m]
    x = x.astype(np.int16)
    g, r = pair(S, O, N, p, S_)
    k0, l0 = S.corr_all_stats()
    got, want = g.stepAll(dev(x), 2), M.step_all(r, x, 2)
    rest, wrest = g.stepAll(dev(x[got[2]:]), 64), M.step_all(r, x[want[2]:], 64)
    k1, l1 = S.corr_all_stats()
    assert (k1 - k0, l1 - l0) == (0, 2)
    assert want[0].tolist() == [700 + (N - 1) * S_, 2500 + (N - 1) * S_] and len(wrest[0]) == 1
    for a, b in ((got, want), (rest, wrest)):
        assert a[0].tolist() == b[0].tolist() and np.array_equal(a[1], b[1]) and a[2] == b[2]
    same_state(g, r, "S4")


def test_equals_the_python_face_loop_of_step_on_clones(S, O):
    for name in ("b2b_32_1", "b2b_64_1", "straddle"):
        N, p, x, _, _ = CASES[name]
        g, _ = pair(S, O, N, p)
        g.step(dev(M.signal(300, 3, [])))  # some history and registers to start from
        twin = copy.copy(g)
        xd = dev(x)
        got, want = g.stepAll(xd, 64), M.step_all(twin, xd, 64)
        assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]) and got[2] == want[2], name
        assert g.getStatus() == twin.getStatus() and np.array_equal(g.getRefBitSamples(), twin.getRefBitSamples())
        extra = dev(M.signal(1500, 5, [(600, p)]))
        assert g.step(extra) == twin.step(extra) == (True, 600 + N - 1), name
        assert g.getStatus() == twin.getStatus()


def test_dropin_member_over_the_c_abi(S, O, tmp_path):
    """dsptl::FixedPatternCorrelator<int16_t, int32_t, 32, 1>::stepAll on host
    vectors (tests/cpp/corr_all_main.cpp), max_hits 3: calls on the remainders."""
    import subprocess
    from srcdsp_amd import _capi
    from test_corr_all_capi import build_dropin
    exe = str(tmp_path / "corr_all_main")
    build_dropin(_capi, exe, stds=("gnu++11",))
    N, p, x, chunks, mh = CASES["max_hits_3"]
    (tmp_path / "p.bin").write_bytes(np.ascontiguousarray(p, np.int32).tobytes())
    (tmp_path / "x.bin").write_bytes(x.tobytes())
    r = subprocess.run([exe, "p.bin", "x.bin", str(mh)], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    ref = O["fma"].corr(N, 1)
    ref.set_pattern(p)
    want = M.run_calls(lambda xs, m: M.step_all(ref, xs, m), x, chunks, mh)
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert [ln for ln in lines[:-2]] == [[w[3]] + w[1] for w in want]
    last = ref.bit_samples().reshape(-1).tolist()
    assert lines[-2] == last and lines[-1] == last


# ------------------------------------------------------------- 4. errors
def test_errors_change_no_state(S, O):
    from srcdsp_amd import _capi as A
    N, p, x, _, _ = CASES["b2b_32_1"]
    gs = [pair(S, O, N, p)[0] for _ in range(2)]
    xd = dev(x)
    S.corr_step_all_batched(gs, xd, 64)
    other_n, other_s = S.FixedPatternCorrelator(64, 1), S.FixedPatternCorrelator(32, 2)
    other_n.setPattern(M.pattern(64, 1))
    other_s.setPattern(M.pattern(32, 2))

    def snapshot():
        return [(g.getStatus(), g.getRefBitSamples().copy()) for g in gs + [other_n, other_s]]

    before, stats = snapshot(), S.corr_all_stats()
    for bad in ([gs[0], other_n], [gs[0], other_s], [gs[0], gs[0]]):
        with pytest.raises(S.SrcdspError) as e:
            S.corr_step_all_batched(bad, xd, 64)
        assert e.value.code == A.ERR_ARG
    for mh in (0, -2):
        with pytest.raises(S.SrcdspError) as e:
            gs[0].stepAll(xd, mh)
        assert e.value.code == A.ERR_ARG
    hs = (C.c_void_p * 2)(*[g._h.value for g in gs])
    k, idx, used = (C.c_int * 2)(5, 5), (C.c_int * 8)(), (C.c_size_t * 2)()
    rc = A.lib().srcdsp_corr_step_all_batched(hs, 2, C.c_void_p(xd.data_ptr()), 0, 1 << 31, 4, k, idx, None, used,
                                              None)
    assert rc == A.ERR_SIZE
    assert A.lib().srcdsp_corr_step_all_batched(hs, 2, None, 0, 0, 4, k, idx, None, used, None) == 0
    assert list(k) == [0, 0] and list(used) == [0, 0]
    with pytest.raises(TypeError):
        S.corr_step_all_batched(gs, x, 4)
    with pytest.raises(ValueError):
        S.corr_step_all_batched(gs, xd[None], 4)
    assert S.corr_all_stats() == stats
    for (s0, b0), (s1, b1) in zip(before, snapshot()):
        assert s0 == s1 and np.array_equal(b0, b1)


# ------------------------------------------------- 5. exact-sqrt build
def test_always_exact_build_gives_the_same_detections(S, O, tmp_path):
    import json
    import subprocess
    import sys
    exact = os.path.join(ROOT, "tests", "_build", "libsrcdsp_hip_corr_exact.so")
    assert os.path.exists(exact), f"{exact} not built: run python -c 'import __graft_entry__ as g; g.build()'"
    out = str(tmp_path / "all_exact.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "corr_all_exact_child.py"), exact, out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["product_mapped"] is False and res["build_flags"] == 1
    assert res["stats"] == [res["calls"], 0] and res["calls"] >= 6
    for name, ev in res["events"].items():
        assert ev == [c[1] for c in run_case(S, O, CASES[name])], name


# --------------------------------- 6. three bursts of one carrier, end to end
def test_three_bursts_in_one_row_end_to_end(S, O):
    """Offset modulator bank -> DDC -> stepAll -> three demodulators, each
    given its burst's bit row, stepped in one launch on the one shared row."""
    import torch
    import corr_all_e2e as E
    import test_gpu_oqpsk_loop as Q
    bits, pre, pay, pattern, idx, base_ref, refs, soft, errs = E.oracle_chain(O["strict"])
    cu, cd = Q.filters()
    tx, rx = S.Mixer(4096), S.Mixer(4096)
    tx.reset(E.FREQ)
    rx.reset(-E.FREQ)
    n_hi = Q.L * (E.NBITS // 2)
    carrier = torch.zeros((1, n_hi, 2), dtype=torch.int16, device="cuda")
    base = torch.zeros((1, n_hi // Q.MDEC, 2), dtype=torch.int16, device="cuda")
    S.modulate_offset_step_batched([S.SymbolMapperQpsk()], [S.FilterUpsamplingFir(cu, Q.L, *Q.I16)], [S.QStagger(Q.D)],
                                   [tx], torch.from_numpy(bits[None]).cuda(), carrier)
    S.mixdecim_step_batched([rx], [S.FilterDnsamplingFir(cd, Q.MDEC, *Q.I16)], carrier, base)
    assert np.array_equal(base[0].cpu().numpy(), base_ref)
    g = S.FixedPatternCorrelator(Q.NPRE, 1)
    g.setPattern(pattern)
    k0, l0 = S.corr_all_stats()
    got_idx, got_bits, used = g.stepAll(base[0], 16)
    assert tuple(b - a for a, b in zip((k0, l0), S.corr_all_stats())) == (1, 0)
    assert got_idx.tolist() == idx and used == base.shape[1]
    # a row the loop detects twice in, two samples apart (the oracle chain at another idle-bit seed)
    other = E.oracle_chain(O["strict"], 3001)
    g2 = S.FixedPatternCorrelator(Q.NPRE, 1)
    g2.setPattern(pattern)
    assert other[4][:2] == [119, 121] and g2.stepAll(dev(other[5]), 16)[0].tolist() == other[4]
    # and stopped by max_hits on the second of them: the registers follow a detection two samples back
    g3, r3 = pair(S, {"fma": O["strict"]}, Q.NPRE, pattern)
    got3, want3 = g3.stepAll(dev(other[5]), 2), M.step_all(r3, other[5], 2)
    assert got3[0].tolist() == want3[0].tolist() == [119, 121] and got3[2] == want3[2] == 123
    same_state(g3, r3, "two apart")
    extra = M.signal(1500, 4243, [(600, pattern)], gain=1)
    assert g3.step(dev(extra)) == r3.step(extra)
    same_state(g3, r3, "two apart, next step")
    demods = []
    for k in range(3):
        ref = Q.remove_modulation(got_bits[k], pattern)
        assert np.array_equal(ref, refs[k]), k
        d = S.DemodulatorOqpsk()
        d.setSyncPattern(pre.astype(np.int8))
        d.setInitialFrequency(0.0)
        d.setReference(ref)
        d.reset()
        demods.append(d)
    sb, ns, er = S.demod_step_batched(demods, base[0], offsets=[i - (Q.NPRE - 1) for i in idx], n=Q.NPRE + Q.NPAY)
    sb = sb.cpu().numpy()
    for k in range(3):
        assert ns[k] == Q.NPAY and np.array_equal(sb[k, :Q.NPAY], soft[k]) and er[k] == errs[k], k
        assert np.array_equal(sb[k, :Q.NPAY] > 0, pay[k] > 0), k
