"""The receive chain with carrier offsets the unseeded PLL cannot take:
correlator bank -> srcdsp_demod_acquire_batched -> demodulator bank.

The join needs correlator handles, which need a device, so its refusals
(`first` out of range, a word outside +-4096, a demodulator taken twice) and
its `found` mask are checked here too."""
import copy

import numpy as np
import pytest

import demod_model as M
import freqest_model as F

pytestmark = pytest.mark.gpu

N = P = 16
C_, NROW, ND, SCALE, SEED = 4, 4000, 300, 0.08, 2027
OMS = (0.08, 0.10, 0.15, 0.0)
PAT = np.tile(np.array([[round(24324 / np.sqrt(N)), 0]], np.int32), (N, 1))  # coeffScaling 14
SYNC = np.ones(P, np.int8)


def build():
    """As tests/test_gpu_demod_chain.py: noise of +-125 and, per row, a burst of
    a bare-carrier preamble of P bit intervals and ND OQPSK bits."""
    rng = np.random.default_rng(SEED)
    x = rng.integers(-125, 126, size=(C_, NROW, 2)).astype(np.int32)
    tx, offs = [], []
    for c in range(C_):
        bits = np.concatenate([SYNC, rng.integers(0, 2, ND).astype(np.int8)])
        th = rng.uniform(-3, 3)
        burst = M.oqpsk_samples(bits, SCALE, OMS[c], th)
        burst[:P] = M.carrier_samples(P, 32572 * SCALE, OMS[c], th)
        off = 500 + 777 * c + c
        x[c, off:off + P + ND] += burst
        tx.append(bits[P:])
        offs.append(off)
    return x.astype(np.int16), tx, offs


def model_demod(bs, f):
    m = M.DemodModel()
    m.set_sync_pattern(SYNC)
    m.set_reference(bs)
    m.set_initial_frequency(f)
    m.reset()
    return m


def cpu_rows(O):
    """The chain on the CPU, with the preconditions that make a bad seed read
    as a bad seed: every burst is detected where it lies, decodes when seeded
    with -estimateFreq over bit samples 1 .. N-1, and does not decode unseeded
    where its offset is not zero."""
    x, tx, offs = build()
    rows = []
    for c in range(C_):
        oc = O["fma"].corr(N, 1)
        oc.set_pattern(PAT)
        hit = oc.step(x[c])
        assert hit == (True, offs[c] + N - 1), ("seed", c, hit)
        bs = np.array(oc.bit_samples(), np.int16).reshape(-1, 2)
        est, sums, exact = F.estimate(bs[1:], 1)
        assert exact
        burst = x[c, offs[c]:offs[c] + P + ND]
        m = model_demod(bs, np.float32(-1.0) * est)
        soft, err = m.step(burst)
        assert np.array_equal(soft > 0, tx[c] > 0), ("seed", c)
        if OMS[c] != 0.0:
            soft0, _ = model_demod(bs, 0.0).step(burst)
            assert not np.array_equal(soft0 > 0, tx[c] > 0), ("seed", c)
            assert abs(float(est) + OMS[c]) < 0.02, (c, est)
        rows.append(dict(hit=hit, bs=bs, est=est, sums=sums, est0=F.estimate(bs, 1)[0], soft=soft, err=err,
                         state=m.state(), word=m.freq))
    return x, tx, offs, rows


@pytest.fixture(scope="module")
def cpu_chain(O):
    return cpu_rows(O)


def handles(S):
    cors, demods = [], []
    for c in range(C_):
        g = S.FixedPatternCorrelator(N, 1)
        g.setPattern(PAT)
        cors.append(g)
        d = S.DemodulatorOqpsk()
        d.setSyncPattern(SYNC)
        demods.append(d)
    return cors, demods


@pytest.fixture(scope="module")
def gpu_hits(S, cpu_chain):
    import torch
    x, tx, offs, rows = cpu_chain
    xd = torch.from_numpy(x).cuda()
    cors, demods = handles(S)
    hits = S.corr_step_batched(cors, xd)
    return xd, cors, demods, hits


def test_acquire_chain_end_to_end(S, cpu_chain, gpu_hits):
    x, tx, offs, rows = cpu_chain
    xd, cors, demods, hits = gpu_hits
    demods = [copy.copy(d) for d in demods]
    assert hits == [r["hit"] for r in rows]
    in_off = [h[1] - (N - 1) for h in hits]
    assert in_off == offs
    est = S.demod_acquire_batched(demods, cors, L=1, first=1, scale=-1.0)
    for c in range(C_):
        assert np.array_equal(cors[c].getRefBitSamples(), rows[c]["bs"]), c
        assert F.bits(est[c]) == F.bits(rows[c]["est"]), c
        assert demods[c].state()[7] == rows[c]["word"] == M.freq_word(np.float32(-1.0) * rows[c]["est"]), c
    soft, ns, errs = S.demod_step_batched(demods, xd, offsets=in_off, n=P + ND)
    soft = soft.cpu().numpy()
    for c in range(C_):
        assert ns[c] == ND and np.array_equal(soft[c, :ND], rows[c]["soft"]) and errs[c] == rows[c]["err"], c
        assert demods[c].state() == rows[c]["state"], c
        assert np.array_equal(soft[c, :ND] > 0, tx[c] > 0), c


def test_device_estimator_over_the_rows_gives_the_join_s_sums(S, cpu_chain, gpu_hits):
    """Bit samples 1 .. N-1 are x[in_off + 1 .. in_off + N - 1]."""
    x, tx, offs, rows = cpu_chain
    xd, cors, demods, hits = gpu_hits
    f, sums, exact = S.FreqEstimator(1).run_batched(xd, offsets=[o + 1 for o in offs], n=N - 1)
    for c in range(C_):
        assert (int(sums[c, 0]), int(sums[c, 1])) == rows[c]["sums"] and exact[c], c
        assert F.bits(f[c]) == F.bits(rows[c]["est"]), c


def test_first_0_is_the_literal_composition(S, cpu_chain, gpu_hits):
    x, tx, offs, rows = cpu_chain
    xd, cors, demods, hits = gpu_hits
    demods = [copy.copy(d) for d in demods]
    est = S.demod_acquire_batched(demods, cors, L=1, first=0, scale=-1.0)
    for c in range(C_):
        assert F.bits(est[c]) == F.bits(rows[c]["est0"]), c
        assert demods[c].state()[7] == M.freq_word(np.float32(-1.0) * rows[c]["est0"]), c
    # L = 2 over bit samples 3 .. N-1
    est = S.demod_acquire_batched(demods, cors, L=2, first=3, scale=-1.0)
    for c in range(C_):
        assert F.bits(est[c]) == F.bits(F.estimate(rows[c]["bs"][3:], 2)[0]), c


def test_join_is_all_or_nothing_and_honours_found(S, cpu_chain, gpu_hits):
    x, tx, offs, rows = cpu_chain
    xd, cors, demods, hits = gpu_hits
    demods = [copy.copy(d) for d in demods]
    for d in demods:
        d.setInitialFrequency(float(M.word_freq(5)))
        d.setInputShift(3)
    before = [d.state() for d in demods]
    for kw in (dict(first=N), dict(first=-1), dict(L=0), dict(scale=100.0)):  # 100 * 0.08 rad: a word past 4096
        with pytest.raises(S.SrcdspError) as ei:
            S.demod_acquire_batched(demods, cors, **kw)
        assert ei.value.code == -1, kw
        assert [d.state() for d in demods] == before, kw
    # channel 3 (offset 0) alone passes the word test with scale = 100: still nothing changed above
    assert abs(100.0 * float(rows[3]["est"])) < 3.0
    with pytest.raises(S.SrcdspError):
        S.demod_acquire_batched([demods[0], demods[1], demods[0], demods[3]], cors)
    assert [d.state() for d in demods] == before
    # found: channels 1 and 3 taken, 0 and 2 untouched and their estimates not written
    est = S.demod_acquire_batched(demods, cors, found=[0, 1, 0, 1])
    assert np.isnan(est[0]) and np.isnan(est[2])
    for c in (0, 2):
        assert demods[c].state() == before[c], c
    for c in (1, 3):
        assert F.bits(est[c]) == F.bits(rows[c]["est"]), c
        m = model_demod(rows[c]["bs"], np.float32(-1.0) * rows[c]["est"])
        assert demods[c].state() == m.state(), c  # reset(): the shift back to 0
    # a demodulator listed twice among channels not taken is not looked at
    S.demod_acquire_batched([demods[0], demods[0], demods[2], demods[3]], cors, found=[0, 0, 0, 1])
