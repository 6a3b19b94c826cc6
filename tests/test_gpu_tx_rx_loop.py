"""Transmit and receive closed on the device: 4 QPSK bursts (a 32-symbol
preamble and 200 payload symbols, each at its own offset in a row of other
symbols) go through the modulator bank (L = 4, each on its own carrier),
straight into the DDC bank at the matching frequencies (M = 4) and the
correlator bank with the preamble's symbols as the pattern.  The GPU chain's
detections equal the same chain through the oracle and the mapper model; a CPU
test pins that the oracle chain finds all four bursts where they lie, so the
GPU test cannot pass on "nothing found anywhere"."""
import numpy as np
import pytest

import mapper_model as M

C_, NPRE, NPAY, NSYM, L, SEED = 4, 32, 200, 600, 4, 2031
FREQS = (0.05, 0.11, -0.07, 0.2)        # carriers, in units of the Nyquist rate after the interpolator
OFFS = (40, 133, 258, 367)              # the burst's first symbol in its row
# the two 32-tap filters' group delay, 2 x 15.5 samples at the high rate: 7.75 symbols, the peak at the 8th
DELAY = 8


def filters():
    from srcdsp_amd.design import hamming_sinc, q14
    # the interpolator at a quarter of unity gain: symbols of +-8192 come out
    # near +-2048, where the correlator's int32 sums (32 products) cannot wrap
    return q14(hamming_sinc(32, 0.48 / L) * L / 4), q14(hamming_sinc(32, 0.48 / L))


def build():
    """Per row: NSYM symbols' worth of bits, the burst's bits at OFFS[c]; the
    preamble is the same for every burst."""
    rng = np.random.default_rng(SEED)
    pre = rng.integers(0, 2, 2 * NPRE).astype(np.uint8)
    bits = rng.choice(np.array([0, 1, 255], np.uint8), size=(C_, 2 * NSYM))
    for c in range(C_):
        burst = np.concatenate([pre, rng.integers(0, 2, 2 * NPAY).astype(np.uint8)])
        bits[c, 2 * OFFS[c]:2 * (OFFS[c] + NPRE + NPAY)] = burst
    # +-3040 per component: sqrt(energy) = 24 320, coeffScaling 14, inside setPattern's energy bound
    pattern = np.sign(M.MapperModel(M.QPSK).step(pre).astype(np.int32)) * 3040
    return bits, pattern


def oracle_chain(o):
    bits, pattern = build()
    cu, cd = filters()
    hits, rx = [], []
    for c in range(C_):
        sym = M.MapperModel(M.QPSK).step(bits[c])
        tx_m = o.mixer(4096)
        tx_m.reset(FREQS[c])
        carrier = tx_m.step(o.up(0, L, cu).step(sym))
        rx_m = o.mixer(4096)
        rx_m.reset(-FREQS[c])
        base = o.decim(1, L, cd).step(rx_m.step(carrier))
        corr = o.corr(NPRE, 1)
        corr.set_pattern(pattern)
        hits.append(corr.step(base))
        rx.append(base)
    return bits, pattern, hits, rx


def test_oracle_chain_finds_all_four_bursts(O):
    bits, pattern, hits, rx = oracle_chain(O["strict"])
    for c in range(C_):
        found, idx = hits[c]
        assert found, c
        # the preamble's last symbol, later by the two filters' delay
        assert idx == OFFS[c] + NPRE - 1 + DELAY, (c, idx)


@pytest.mark.gpu
def test_gpu_chain_equals_the_oracle_chain(S, O):
    import torch
    bits, pattern, hits, rx = oracle_chain(O["strict"])
    cu, cd = filters()
    i16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")
    maps = [S.SymbolMapperQpsk() for _ in range(C_)]
    ups = [S.FilterUpsamplingFir(cu, L, *i16) for _ in range(C_)]
    tx, rxm, decims, cors = [], [], [], []
    for c in range(C_):
        for lst, f in ((tx, FREQS[c]), (rxm, -FREQS[c])):
            m = S.Mixer(4096)
            m.reset(f)
            lst.append(m)
        decims.append(S.FilterDnsamplingFir(cd, L, *i16))
        g = S.FixedPatternCorrelator(NPRE, 1)
        g.setPattern(pattern)
        cors.append(g)
    bd = torch.from_numpy(bits).cuda()
    carrier = torch.zeros((C_, L * NSYM, 2), dtype=torch.int16, device="cuda")
    base = torch.zeros((C_, NSYM, 2), dtype=torch.int16, device="cuda")
    s0 = S.modulate_stats()
    S.modulate_step_batched(maps, ups, tx, bd, carrier)
    assert tuple(b - a for a, b in zip(s0, S.modulate_stats())) == (0, 0, 1, 0)
    S.mixdecim_step_batched(rxm, decims, carrier, base)
    got = S.corr_step_batched(cors, base)
    assert got == hits
    assert all(f for f, _ in got)
    y = base.cpu().numpy()
    for c in range(C_):
        assert np.array_equal(y[c], np.asarray(rx[c]).reshape(-1, 2)), c
