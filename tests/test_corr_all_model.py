"""The definition of srcdsp_corr_step_all on the CPU: the oracle loop
(corr_all_model.step_all over O["fma"].corr) finds the planted bursts where
they lie; on back-to-back preambles its detections differ from the points
where the peak test fires on the undisturbed stream; and the two properties
the kernels rest on hold in the oracle's registers."""
import numpy as np
import pytest

import corr_all_model as M


def _ref(O, N, p, S_=1):
    r = O["fma"].corr(N, S_)
    r.set_pattern(p)
    return r


def _loop(O, N, p, x, mh=1000):
    return M.step_all(_ref(O, N, p), x, mh)


def test_the_loop_finds_the_planted_bursts(O):
    for name, (N, p, x, chunks, mh) in M.cases().items():
        if name.startswith("tile_"):
            q = int(name.split("_")[1])
            idx, bits, used = _loop(O, N, p, x)
            assert idx.tolist() == [q - 1, q + 700 + N - 1, q + 2500 + N - 1], (name, idx)
            assert used == len(x) and bits.shape == (3, N, 2)
            # the bitSamples of a detection: the N samples ending at the peak, the oldest replaced by the detected one
            want = x[q - N:q].copy()
            want[0] = x[q]
            assert np.array_equal(bits[0], want), name
    p, x = M.tile_row(33, M.TILE + 1, 633)
    assert _loop(O, 33, p, x)[0].tolist()[0] == M.TILE


def test_back_to_back_detections_differ_from_the_firing_points(O):
    """The case of the issue: N = 32, gaps 0, 0, 0, 1, 1, 2, 5, 40.  The test
    fires after every preamble; the loop misses the second and the fourth."""
    p, x, offs = M.back_to_back(32, 1)
    fire = M.firing_points(_ref(O, 32, p), x)
    assert fire == [o + 32 for o in offs] == [532, 564, 596, 628, 661, 694, 728, 765, 837]
    idx, _, used = _loop(O, 32, p, x)
    assert (idx + 1).tolist() == [532, 596, 661, 694, 728, 765, 837] and used == len(x)
    p, x, offs = M.back_to_back(64, 3)
    assert M.firing_points(_ref(O, 64, p), x) == [o + 64 for o in offs]
    assert (_loop(O, 64, p, x)[0] + 1).tolist() == [564, 692, 821, 886, 952, 1021, 1125]
    # and rows where a detection inside the stretch a deletion disturbs is made
    for N, seed in ((32, 4), (64, 1)):
        p, x, offs = M.back_to_back(N, seed)
        assert (_loop(O, N, p, x)[0] + 1).tolist() == [o + N for o in offs], (N, seed)


def test_straddle_row_detects_inside_a_patch_across_the_tile_boundary(O):
    N, p, x, _, _ = M.cases()["straddle"]
    q = (_loop(O, N, p, x)[0] + 1).tolist()
    assert q[0] == M.TILE - 6 and q[1] == M.TILE - 6 + N, q  # q[1] <= q[0] + N + 1: inside the patch


def test_split_row_has_a_detection_at_a_calls_first_sample(O):
    N, p, x, chunks, mh = M.cases()["split"]
    r = _ref(O, N, p)
    calls = M.run_calls(lambda xs, m: M.step_all(r, xs, m), x, chunks, mh)
    assert calls[0][1] == [531] and calls[1][1] == [] and calls[2][1][0] == -1, [c[1] for c in calls]


def test_max_hits_calls_add_up_to_one_call(O):
    cs = M.cases()
    N, p, x, chunks, _ = cs["max_hits_exact"]
    whole = _loop(O, N, p, x)
    assert len(whole[0]) == 7
    for name in ("max_hits_3", "max_hits_exact"):
        mh = cs[name][4]
        r = _ref(O, N, p)
        calls = M.run_calls(lambda xs, m: M.step_all(r, xs, m), x, chunks, mh)
        assert [len(c[1]) for c in calls] == ([3, 3, 1] if mh == 3 else [7, 0]), name
        assert [c[0] + i for c in calls for i in c[1]] == whole[0].tolist(), name
        assert np.array_equal(np.concatenate([c[2] for c in calls]), whole[1]), name
        assert calls[0][3] == calls[0][1][-1] + 2  # consumed: one past the detected sample
        assert r.status() == M.step_all_status(O, N, p, x)


def test_oracle_chain_finds_and_decodes_three_bursts_of_one_row(O):
    import corr_all_e2e as E
    import test_gpu_oqpsk_loop as Q
    bits, pre, pay, pattern, idx, base, refs, soft, errs = E.oracle_chain(O["strict"])
    # each preamble's last bit sample, later by the two filters' delay
    assert idx == [2 * f + Q.DELAY + Q.NPRE - 1 for f in E.OFFS]
    for k in range(3):
        assert len(soft[k]) == Q.NPAY and int(((soft[k] > 0) != (pay[k] > 0)).sum()) == 0, k
    # and a seed whose row the loop detects twice in, two samples apart
    assert E.oracle_chain(O["strict"], 3001)[4][:2] == [119, 121]


@pytest.mark.parametrize("S_", [1, 4])
def test_the_two_properties_in_the_oracles_registers(O, S_):
    """After a detection while processing sample q: (1) the registers from
    q + 1 on are those of a fresh correlator over the stream with sample q
    deleted; (2) from q + (N - 1) S + 1 on corrValue[0] and energyValue[0] are
    the undisturbed stream's again."""
    N = 32
    p = M.pattern(N, 21)
    rng = np.random.default_rng(22)
    x = rng.integers(-125, 126, size=(3000, 2)).astype(np.int32)
    for m in range(N):
        x[700 + m * S_] += 2 * p[m]
    x = x.astype(np.int16)
    r = _ref(O, N, p, S_)
    found, ci = r.step(x)
    assert found and ci == 700 + (N - 1) * S_
    q = ci + 1
    c_after, e_after = r.registers(x[q + 1:])                      # the loop's correlator, going on
    c_del, e_del = _ref(O, N, p, S_).registers(np.delete(x, q, axis=0))
    assert np.array_equal(c_after, c_del[q:]) and np.array_equal(e_after, e_del[q:])  # (1)
    c_und, e_und = _ref(O, N, p, S_).registers(x)
    first = q + (N - 1) * S_ + 1
    assert np.array_equal(c_after[first - (q + 1):], c_und[first:])                  # (2)
    assert np.array_equal(e_after[first - (q + 1):], e_und[first:])
    assert not np.array_equal(c_after[:first - (q + 1)], c_und[q + 1:first])         # and not before
