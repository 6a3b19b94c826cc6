"""The receive chain's last two stages on the device: correlator bank ->
demodulator bank, joined by srcdsp_demod_set_reference_corr."""
import numpy as np
import pytest

import demod_model as M

pytestmark = pytest.mark.gpu


def test_receive_chain_end_to_end(S, O):
    """4 channels, N = P = 32, S = 1, 4000 samples a row: noise of +-125 and,
    at another place in each row, a burst with its own carrier phase and
    frequency offset -- a preamble of 32 bit intervals, then 300 OQPSK bits of
    the signal model the demodulator reconstructs (demodulators.cpp:217-235).

    The preamble is sent as the bare carrier: setReference expects the sync
    word's bit samples with the modulation removed (demodulators.h:97-99), and
    the join hands the correlator's bit samples over as they are.  The
    correlator's pattern is therefore constant, its amplitude chosen for
    coeffScaling = 14 (sqrt(32) * 4300 = 24 324 in [2^14, 2^15)), where a clean
    match passes the threshold test with margin.

    srcdsp_corr_step_batched finds every burst.  With S = 1 the reference
    detects one sample after the peak and reports corrIndex = the peak, the
    preamble's last sample (correlators.h:262-276); bitSamples[m] for m >= 1 is
    the ring read backwards from the peak, x[corrIndex - (N - 1) + m], and
    bitSamples[0] is the slot the detected sample already overwrote,
    x[corrIndex + 1] (correlators.h:278-288).  The preamble's first sample is
    therefore at in_offset = corrIndex - (N - 1), and from there each channel
    is stepped P + 300 samples by srcdsp_demod_step_batched.  The same chain
    run per channel through the oracle correlator and the model gives the same
    soft bits, and their signs are the transmitted bits."""
    N = P = 32
    C_, n, nd, scale = 4, 4000, 300, 0.08
    rng = np.random.default_rng(2026)
    pat = np.tile(np.array([[4300, 0]], np.int32), (N, 1))
    sync = np.ones(P, np.int8)
    oms = (0.01, -0.006, 0.0, 0.004)
    x = rng.integers(-125, 126, size=(C_, n, 2)).astype(np.int32)
    tx, offs = [], []
    for c in range(C_):
        bits = np.concatenate([sync, rng.integers(0, 2, nd).astype(np.int8)])
        th = rng.uniform(-3, 3)
        burst = M.oqpsk_samples(bits, scale, oms[c], th)
        burst[:P] = M.carrier_samples(P, 32572 * scale, oms[c], th)
        off = 500 + 777 * c + c
        x[c, off:off + P + nd] += burst
        tx.append(bits[P:])
        offs.append(off)
    x = x.astype(np.int16)
    import torch
    xd = torch.from_numpy(x).cuda()

    cors, demods = [], []
    for c in range(C_):
        g = S.FixedPatternCorrelator(N, 1)
        g.setPattern(pat)
        cors.append(g)
        d = S.DemodulatorOqpsk()
        d.setSyncPattern(sync)
        d.setInitialFrequency(0.0)
        demods.append(d)
    hits = S.corr_step_batched(cors, xd)
    in_off = []
    for c in range(C_):
        oc = O["fma"].corr(N, 1)
        oc.set_pattern(pat)
        assert hits[c] == oc.step(x[c]) == (True, offs[c] + N - 1), c
        in_off.append(hits[c][1] - (N - 1))
        demods[c].setReference(cors[c])       # srcdsp_demod_set_reference_corr
        demods[c].reset()
        bs = oc.bit_samples()
        assert np.array_equal(bs[1:], x[c, in_off[c] + 1:in_off[c] + N]) and np.array_equal(bs[0], x[c, in_off[c] + N])
    assert in_off == offs
    soft, ns, errs = S.demod_step_batched(demods, xd, offsets=in_off, n=P + nd)
    soft = soft.cpu().numpy()
    for c in range(C_):
        m = M.DemodModel()
        m.set_sync_pattern(sync)
        m.set_reference(cors[c].getRefBitSamples())
        m.set_initial_frequency(0.0)
        m.reset()
        want, werr = m.step(x[c, in_off[c]:in_off[c] + P + nd])
        assert ns[c] == nd == len(want) and np.array_equal(soft[c, :nd], want) and errs[c] == werr, c
        assert demods[c].state() == m.state(), c
        assert np.array_equal(soft[c, :nd] > 0, tx[c] > 0), c
        assert abs(demods[c].getMeasuredFrequency() - oms[c]) < 2 * np.pi / 4096, c
