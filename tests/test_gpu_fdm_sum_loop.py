"""Offset-QPSK sent and decoded over ONE wire with the transmit side in one
call: the chain of tests/test_gpu_fdm_loop.py (its bursts, carriers, filters
and oracle chain) with srcdsp_modulate_sum_step in place of the offset
modulator bank followed by the carrier combiner.  The wire leaves the fused
kernel (every call it takes is routed to it for the test: the measured routing
sends no call at L = 8 there), equals the oracle chain's composite, the
transmit handles end as the oracle chain's, and the unchanged receive bank
(DDC with the wire as its shared input, correlators, demodulators) decodes all
4 x 300 payload bits."""
import numpy as np
import pytest

from test_gpu_fdm_loop import FREQS, SHIFTS, oracle_chain
from test_gpu_oqpsk_loop import C_, D, I16, L, MDEC, NBITS, NPAY, NPRE, filters, remove_modulation


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
def test_one_call_from_bits_to_the_wire_and_back(S, O, shift):
    import torch
    r = oracle_chain(O["strict"], shift)
    bits, pre, pay, pattern = r["bits"], r["pre"], r["pay"], r["pattern"]
    assert sum(len(p) for p in pay) == 4 * 300
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
    wire = torch.zeros((n_hi, 2), dtype=torch.int16, device="cuda")  # ONE row, and no carrier rows
    s0 = S.modulate_sum_stats()
    S.modulate_sum_set_min_tiles(1)
    try:
        assert S.modulate_sum_step(maps, ups, stags, tx, bd, wire, shift) is wire
    finally:
        S.modulate_sum_set_min_tiles(0)
    # the fused kernel served it, not the bank and the combiner
    assert tuple(b - a for a, b in zip(s0, S.modulate_sum_stats())) == (1, 0)
    assert np.array_equal(wire.cpu().numpy(), r["wire"])
    for c in range(C_):
        state = {"mixer": tuple(tx[c].state()[:2]), "mapper": maps[c].state(), "carry": stags[c].state().tolist()}
        assert state == r["tx"][c], c
    base = torch.zeros((C_, n_hi // MDEC, 2), dtype=torch.int16, device="cuda")
    S.mixdecim_step_batched(rxm, decims, wire, base)  # the composite as the shared input
    got = S.corr_step_batched(cors, base)
    assert got == r["hits"] and all(f for f, _ in got)
    in_off = []
    for c in range(C_):
        demods[c].setReference(remove_modulation(cors[c].getRefBitSamples(), pattern))
        demods[c].reset()
        in_off.append(got[c][1] - (NPRE - 1))
    sb, ns, er = S.demod_step_batched(demods, base, offsets=in_off, n=NPRE + NPAY)
    sb = sb.cpu().numpy()
    for c in range(C_):
        assert ns[c] == NPAY == len(r["soft"][c]) and np.array_equal(sb[c, :NPAY], r["soft"][c]), c
        assert np.array_equal(sb[c, :NPAY] > 0, pay[c] > 0), c  # every payload bit
