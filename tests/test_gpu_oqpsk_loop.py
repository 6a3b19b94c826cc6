"""Offset-QPSK sent and decoded on the device: the bits sent are the bits
decoded.  4 bursts (a 32-bit preamble and 300 payload bits, each at its own
offset in a row of idle bits) go through the offset modulator bank (QPSK
mapper, L = 8, the Q rail delayed by D = 4 samples = one bit interval, each on
its own carrier), straight into the DDC bank at the negated frequencies (M = 4:
one sample per bit), the correlator bank with the preamble's OQPSK bit samples
as the pattern, and from each hit the demodulator bank.  Removing the
preamble's modulation from the correlator's bit samples is the application's
part and is done on the host here.

The GPU chain's detections, soft bits, error sums and demodulator states equal
the same chain through the oracle, the mapper, stagger and demodulator models;
a CPU test pins that this chain finds all four bursts where they lie and
decodes them with no bit error, so the GPU test cannot pass on "nothing
found".

The idle bits around the bursts are random, and a correlator at its default
threshold may fire on them before the burst: through the oracle chain, with the
draw order of build(), the idle-bit seeds 2031 and 2035 give all four hits
where the bursts lie, while 2033, 2034 and 2036 give some row an earlier false
detection.  The seed is chosen from the oracle chain alone; what the GPU
computes has no part in it."""
import numpy as np
import pytest

import demod_model as DM
import mapper_model as M
import stagger_model as G

C_, NBITS, NPRE, NPAY, L, D, MDEC, SEED = 4, 1200, 32, 300, 8, 4, 4, 2031
FREQS = (0.05, 0.11, -0.07, 0.2)    # carriers, in units of the Nyquist rate after the interpolator
OFFS = (40, 133, 258, 367)          # the burst's first symbol in its row; its first bit sample is 2 * OFFS
# the two filters' group delay, 15 + 16 samples at the high rate: 7.75 bit intervals, the peak at the 8th
DELAY = 8
I16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")


def filters():
    from srcdsp_amd.design import hamming_sinc, q14
    cu = np.concatenate([q14(hamming_sinc(31, 0.06)), np.zeros(1, np.int32)])  # a whole number of taps per phase
    return cu, q14(hamming_sinc(33, 0.09))


def build():
    """Per row NBITS bits, the burst's bits from bit 2 * OFFS[c]; the preamble
    is the same for every burst.  The correlator's pattern is the signal the
    demodulator itself reconstructs for the preamble, one sample per bit,
    scaled to sqrt(energy) = 24 324 (coeffScaling 14, inside setPattern's
    energy bound)."""
    rng = np.random.default_rng(SEED)
    pre = np.random.default_rng(5).integers(0, 2, NPRE).astype(np.uint8)
    bits, pay = np.zeros((C_, NBITS), np.uint8), np.zeros((C_, NPAY), np.uint8)
    for c in range(C_):  # row by row: its idle bits, then its payload
        bits[c] = rng.choice(np.array([0, 1, 255], np.uint8), NBITS)
        pay[c] = rng.integers(0, 2, NPAY)
        bits[c, 2 * OFFS[c]:2 * OFFS[c] + NPRE + NPAY] = np.concatenate([pre, pay[c]])
    s = DM.oqpsk_samples(pre, 1.0).astype(np.float64)
    pattern = np.round(s * (24324.0 / np.sqrt((s * s).sum()))).astype(np.int32)
    return bits, pre, pay, pattern


def remove_modulation(bit_samples, pattern):
    """The sync word's bit samples with the modulation removed, as setReference
    takes them (demodulators.h:97-99): (bitSamples * conj(pattern)) >> 13."""
    b, p = np.asarray(bit_samples, np.int64).reshape(-1, 2), np.asarray(pattern, np.int64).reshape(-1, 2)
    re = b[:, 0] * p[:, 0] + b[:, 1] * p[:, 1]
    im = b[:, 1] * p[:, 0] - b[:, 0] * p[:, 1]
    ref = np.stack([re >> 13, im >> 13], 1)
    assert np.abs(ref).max() < 32768
    return ref.astype(np.int16)


def oracle_chain(o):
    bits, pre, pay, pattern = build()
    cu, cd = filters()
    hits, rx, refs, soft, errs, states = [], [], [], [], [], []
    for c in range(C_):
        tx_m, rx_m = o.mixer(4096), o.mixer(4096)
        tx_m.reset(FREQS[c])
        rx_m.reset(-FREQS[c])
        y = np.asarray(o.up(0, L, cu).step(M.MapperModel(M.QPSK).step(bits[c]))).reshape(-1, 2)
        carrier = tx_m.step(G.StaggerModel(D).step(y))
        base = np.asarray(o.decim(1, MDEC, cd).step(rx_m.step(carrier))).reshape(-1, 2)
        corr = o.corr(NPRE, 1)
        corr.set_pattern(pattern)
        hit = corr.step(base)
        hits.append(hit)
        rx.append(base)
        ref = remove_modulation(corr.bit_samples(), pattern)
        refs.append(ref)
        m = DM.DemodModel()
        m.set_sync_pattern(pre)
        m.set_reference(ref)
        m.set_initial_frequency(0.0)
        m.reset()
        first = hit[1] - (NPRE - 1)
        sb, e = m.step(base[first:first + NPRE + NPAY]) if hit[0] else (np.zeros(0, np.int8), 0)
        soft.append(sb)
        errs.append(e)
        states.append(m.state())
    return bits, pre, pay, pattern, hits, rx, refs, soft, errs, states


def test_oracle_chain_finds_and_decodes_all_four_bursts(O):
    bits, pre, pay, pattern, hits, rx, refs, soft, errs, states = oracle_chain(O["strict"])
    for c in range(C_):
        found, idx = hits[c]
        assert found, c
        # the preamble's last bit sample, later by the two filters' delay
        assert idx == 2 * OFFS[c] + DELAY + NPRE - 1, (c, idx)
        assert len(soft[c]) == NPAY
        assert int(((soft[c] > 0) != (pay[c] > 0)).sum()) == 0, c
        # the decimator's output is near +-4950 inside the burst
        first = idx - (NPRE - 1)
        amp = np.abs(rx[c][first:first + NPRE + NPAY].astype(np.int32)).max()
        assert 4000 < amp < 8000, (c, amp)


@pytest.mark.gpu
def test_gpu_chain_equals_the_oracle_chain(S, O):
    import torch
    bits, pre, pay, pattern, hits, rx, refs, soft, errs, states = oracle_chain(O["strict"])
    cu, cd = filters()
    maps = [S.SymbolMapperQpsk() for _ in range(C_)]
    ups = [S.FilterUpsamplingFir(cu, L, *I16) for _ in range(C_)]
    stags = [S.QStagger(D) for _ in range(C_)]
    tx, rxm, decims, cors, demods = [], [], [], [], []
    for c in range(C_):
        for lst, f in ((tx, FREQS[c]), (rxm, -FREQS[c])):
            m = S.Mixer(4096)
            m.reset(f)
            lst.append(m)
        decims.append(S.FilterDnsamplingFir(cd, MDEC, *I16))
        g = S.FixedPatternCorrelator(NPRE, 1)
        g.setPattern(pattern)
        cors.append(g)
        d = S.DemodulatorOqpsk()
        d.setSyncPattern(pre.astype(np.int8))
        d.setInitialFrequency(0.0)
        demods.append(d)
    n_hi = L * (NBITS // 2)
    bd = torch.from_numpy(bits).cuda()
    carrier = torch.zeros((C_, n_hi, 2), dtype=torch.int16, device="cuda")
    base = torch.zeros((C_, n_hi // MDEC, 2), dtype=torch.int16, device="cuda")
    s0 = S.modulate_offset_stats()
    S.modulate_offset_step_batched(maps, ups, stags, tx, bd, carrier)
    # the modulator bank took its one-launch path
    assert tuple(b - a for a, b in zip(s0, S.modulate_offset_stats())) == (0, 0, 1, 0)
    S.mixdecim_step_batched(rxm, decims, carrier, base)
    got = S.corr_step_batched(cors, base)
    assert got == hits and all(f for f, _ in got)
    y = base.cpu().numpy()
    in_off = []
    for c in range(C_):
        assert np.array_equal(y[c], rx[c]), c
        ref = remove_modulation(cors[c].getRefBitSamples(), pattern)  # on the host: the application's part
        assert np.array_equal(ref, refs[c]), c
        demods[c].setReference(ref)
        demods[c].reset()
        in_off.append(got[c][1] - (NPRE - 1))
    sb, ns, er = S.demod_step_batched(demods, base, offsets=in_off, n=NPRE + NPAY)
    sb = sb.cpu().numpy()
    for c in range(C_):
        assert ns[c] == NPAY == len(soft[c]) and np.array_equal(sb[c, :NPAY], soft[c]) and er[c] == errs[c], c
        assert demods[c].state() == states[c], c
        assert np.array_equal(sb[c, :NPAY] > 0, pay[c] > 0), c
