"""Offset-QPSK sent and decoded over ONE wire: the four bursts of
tests/test_gpu_oqpsk_loop.py (its bits, filters, preamble and pattern), each on
its own carrier, leave the offset modulator bank in four rows and are summed
by the carrier combiner (srcdsp_combine_step) into one composite row; that row is the
SHARED input of the DDC bank at the negated frequencies (the bank kernel that
reads its input once, in_stride == 0), then the correlator bank, the host's
remove_modulation and the demodulator bank.

The carriers are (-0.6, -0.2, 0.2, 0.6): the frequencies of the four private
links of test_gpu_oqpsk_loop overlap once they share a wire.  The GPU chain's
composite, DDC rows, detections, references, soft bits, error sums and
demodulator states equal the same chain through the oracle and the models; a
CPU test pins that this chain finds all four bursts where they lie, decodes
them with no bit error and does not saturate the composite, so the GPU test
cannot pass on "nothing found" or on a clipped wire."""
import numpy as np
import pytest

import demod_model as DM
import mapper_model as M
from combine_model import combine as combine_model
from test_gpu_oqpsk_loop import (C_, D, DELAY, I16, L, MDEC, NBITS, NPAY, NPRE, OFFS, build, filters,
                                 remove_modulation)
from tx_chain_model import MODULATE_OFFSET, TxChain

FREQS = (-0.6, -0.2, 0.2, 0.6)   # a spacing of 0.4: at 0.3 one payload bit is decoded wrong
SHIFTS = (0, 2)
_CHAIN = {}


def oracle_chain(o, shift):
    """Computed once per shift and shared; nothing in it is changed later."""
    if shift in _CHAIN:
        return _CHAIN[shift]
    bits, pre, pay, pattern = build()
    cu, cd = filters()
    tx = [TxChain(o, MODULATE_OFFSET, L, cu, 4096, FREQS[c], M.QPSK, D) for c in range(C_)]
    rows = np.stack([tx[c].step(bits[c]) for c in range(C_)])
    total = rows.astype(np.int64).sum(0)
    wire = combine_model(rows, shift)
    hits, rx, refs, soft, errs, states = [], [], [], [], [], []
    for c in range(C_):
        rx_m = o.mixer(4096)
        rx_m.reset(-FREQS[c])
        base = np.asarray(o.decim(1, MDEC, cd).step(rx_m.step(wire))).reshape(-1, 2)
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
    _CHAIN[shift] = dict(bits=bits, pre=pre, pay=pay, pattern=pattern, tx=[t.state() for t in tx], total=total,
                         wire=wire, hits=hits, rx=rx, refs=refs, soft=soft, errs=errs, states=states)
    return _CHAIN[shift]


@pytest.mark.parametrize("shift", SHIFTS)
def test_oracle_chain_decodes_all_four_bursts_from_one_wire(O, shift):
    r = oracle_chain(O["strict"], shift)
    # the composite does not saturate: the sum of four carriers stays inside int16
    peak = int(np.abs(r["total"]).max())
    assert 20000 < peak < 32767, peak
    assert np.array_equal(r["wire"].astype(np.int64), r["total"] >> shift)
    for c in range(C_):
        found, idx = r["hits"][c]
        assert found, c
        assert idx == 2 * OFFS[c] + DELAY + NPRE - 1, (c, idx)
        assert len(r["soft"][c]) == NPAY
        assert int(((r["soft"][c] > 0) != (r["pay"][c] > 0)).sum()) == 0, c  # a condition, not a tolerance
        first = idx - (NPRE - 1)
        amp = np.abs(r["rx"][c][first:first + NPRE + NPAY].astype(np.int32)).max()
        assert 4000 >> shift < amp < 8000 >> shift, (c, amp)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
def test_gpu_chain_over_one_wire_equals_the_oracle_chain(S, O, shift):
    import torch
    r = oracle_chain(O["strict"], shift)
    bits, pre, pay, pattern = r["bits"], r["pre"], r["pay"], r["pattern"]
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
    wire = torch.zeros((n_hi, 2), dtype=torch.int16, device="cuda")  # ONE row
    base = torch.zeros((C_, n_hi // MDEC, 2), dtype=torch.int16, device="cuda")
    carriers = torch.zeros((C_, n_hi, 2), dtype=torch.int16, device="cuda")
    S.modulate_offset_step_batched(maps, ups, stags, tx, bd, carriers)
    assert S.combine(carriers, wire, shift) is wire
    assert np.array_equal(wire.cpu().numpy(), r["wire"])
    for c in range(C_):
        state = {"mixer": tuple(tx[c].state()[:2]), "mapper": maps[c].state(), "carry": stags[c].state().tolist()}
        assert state == r["tx"][c], c
    d0 = S.mixdecim_batched_stats()
    S.mixdecim_step_batched(rxm, decims, wire, base)  # the composite as the shared input
    # the bank kernel served it, not the per-channel loop
    assert tuple(b - a for a, b in zip(d0, S.mixdecim_batched_stats())) == (1, 0)
    got = S.corr_step_batched(cors, base)
    assert got == r["hits"] and all(f for f, _ in got)
    y = base.cpu().numpy()
    in_off = []
    for c in range(C_):
        assert np.array_equal(y[c], r["rx"][c]), c
        ref = remove_modulation(cors[c].getRefBitSamples(), pattern)  # on the host: the application's part
        assert np.array_equal(ref, r["refs"][c]), c
        demods[c].setReference(ref)
        demods[c].reset()
        in_off.append(got[c][1] - (NPRE - 1))
    sb, ns, er = S.demod_step_batched(demods, base, offsets=in_off, n=NPRE + NPAY)
    sb = sb.cpu().numpy()
    for c in range(C_):
        assert ns[c] == NPAY == len(r["soft"][c]) and np.array_equal(sb[c, :NPAY], r["soft"][c]), c
        assert er[c] == r["errs"][c] and demods[c].state() == r["states"][c], c
        assert np.array_equal(sb[c, :NPAY] > 0, pay[c] > 0), c
