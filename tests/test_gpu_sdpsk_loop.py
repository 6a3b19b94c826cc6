"""SDPSK sent and decoded on the device: the bits sent are the bits decoded.

Private links: the setup of tests/test_gpu_tx_rx_loop.py (its filters, carriers,
L = M = 4, offsets, a 32-symbol preamble and 200 payload symbols) with the SDPSK
mapper and rows of 640 bits.  Modulator bank -> DDC bank -> correlator bank
(the pattern is the preamble's own symbols' signs x 3040) -> SDPSK demodulator
bank at D = 1, every row from its hit.

One wire: L = 8, 64 taps on both sides, the four carriers of
tests/test_gpu_fdm_loop.py summed by the carrier combiner at shift 2, and the
composite as the DDC bank's shared input, received twice: at M = 8 (one sample
per symbol, an S = 1 correlator, D = 1) and at M = 4 (two samples per symbol,
an S = 2 correlator, D = 2: the demodulator bank's outputs are read every
second sample from the hit).

Each loop has a CPU half that pins the chain through the oracle and the models:
every hit lies where the burst lies, no payload bit is decoded wrong, the
composite stays inside int16.  So the GPU half, which asserts that hits, DDC
rows, soft bits, bits and carries equal that chain, cannot pass on "nothing
found".

The idle bits around the bursts are random and a correlator at its default
threshold may fire on them before the burst.  The seeds were chosen from the
oracle chain alone, with the draw order of build(): the private links hold
their conditions for every seed 2031 ... 2035 and keep the sibling test's
2031; over one wire 2031 and 2035 give a row an early false detection and
2032, 2033 and 2034 give all hits where the bursts lie and no bit error in both
receivers: 2032.  What the GPU computes has no part in it."""
import numpy as np
import pytest

import mapper_model as M
from combine_model import combine as combine_model
from sdpsk_model import SdpskModel, tq_of
from test_gpu_tx_rx_loop import C_, DELAY, FREQS, NPAY, NPRE, OFFS
from test_gpu_tx_rx_loop import L as L_LINK
from test_gpu_tx_rx_loop import filters as link_filters

NBITS = 640
I16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")
LINK_SEED, LINK_SHIFT = 2031, 19  # |tq| inside the bursts is 7.7e6 ... 3.66e7: |soft| >= 14, unclamped
WIRE_SEED, WIRE_SHIFT, WIRE_L, COMBINE_SHIFT = 2032, 17, 8, 2  # |tq| 2.8e6 ... 9.3e6: |soft| 21 ... 70
WIRE_FREQS = (-0.6, -0.2, 0.2, 0.6)
# (M, the correlator's S = the demodulator's D = samples per symbol)
RECEIVERS = ((8, 1), (4, 2))
_CHAIN = {}


def wire_filters():
    from srcdsp_amd.design import hamming_sinc, q14
    return q14(hamming_sinc(64, 0.48 / WIRE_L) * WIRE_L / 4), q14(hamming_sinc(64, 0.48 / WIRE_L))


def build(seed):
    """Per row NBITS bits (one SDPSK symbol each), the burst's bits from bit
    OFFS[c]; the preamble is the same for every burst."""
    rng = np.random.default_rng(seed)
    pre = rng.integers(0, 2, NPRE).astype(np.uint8)
    bits = rng.choice(np.array([0, 1, 255], np.uint8), size=(C_, NBITS))
    pay = np.zeros((C_, NPAY), np.uint8)
    for c in range(C_):
        pay[c] = rng.integers(0, 2, NPAY)
        bits[c, OFFS[c]:OFFS[c] + NPRE + NPAY] = np.concatenate([pre, pay[c]])
    # +-3040 per component: sqrt(energy) = 24 320, coeffScaling 14, inside setPattern's energy bound
    pattern = np.sign(M.MapperModel(M.SDPSK).step(pre).astype(np.int32)) * 3040
    return bits, pre, pay, pattern


def receive(o, x, freq, cd, Mdec, sps, pattern, shift):
    """One receiver of one carrier: DDC, correlator, and from the hit the SDPSK
    model over the payload, its window D samples early."""
    rx_m = o.mixer(4096)
    rx_m.reset(-freq)
    base = np.asarray(o.decim(1, Mdec, cd).step(rx_m.step(x))).reshape(-1, 2)
    corr = o.corr(NPRE, sps)
    corr.set_pattern(pattern)
    hit = corr.step(base)
    r = dict(base=base, hit=hit, soft=None, bits=None, carry=None, whole=SdpskModel(sps, shift).step(base)[1])
    if hit[0]:
        m = SdpskModel(sps, shift)
        first = hit[1]  # the first payload sample is hit + sps, and the window starts D = sps samples early
        r["first"], r["n"] = first, sps * NPAY + sps
        r["soft"], r["bits"] = m.step(base[first:first + r["n"]])
        r["carry"] = m.carry
        r["tq"] = np.abs(tq_of(base[first + sps:first + r["n"]:sps], base[first:first + r["n"] - sps:sps]))
    return r


def link_chain(o, seed=LINK_SEED):
    """Computed once and shared; nothing in it is changed later."""
    if ("link", seed) in _CHAIN:
        return _CHAIN["link", seed]
    bits, pre, pay, pattern = build(seed)
    cu, cd = link_filters()
    rows = []
    for c in range(C_):
        tx_m = o.mixer(4096)
        tx_m.reset(FREQS[c])
        carrier = tx_m.step(o.up(0, L_LINK, cu).step(M.MapperModel(M.SDPSK).step(bits[c])))
        rows.append(receive(o, carrier, FREQS[c], cd, L_LINK, 1, pattern, LINK_SHIFT))
    _CHAIN["link", seed] = dict(bits=bits, pre=pre, pay=pay, pattern=pattern, rows=rows)
    return _CHAIN["link", seed]


def wire_chain(o, seed=WIRE_SEED):
    if ("wire", seed) in _CHAIN:
        return _CHAIN["wire", seed]
    bits, pre, pay, pattern = build(seed)
    cu, cd = wire_filters()
    carriers = []
    for c in range(C_):
        tx_m = o.mixer(4096)
        tx_m.reset(WIRE_FREQS[c])
        carriers.append(np.asarray(tx_m.step(o.up(0, WIRE_L, cu).step(M.MapperModel(M.SDPSK).step(bits[c])))).reshape(-1, 2))
    carriers = np.stack(carriers)
    total = carriers.astype(np.int64).sum(0)
    wire = combine_model(carriers, COMBINE_SHIFT)
    rx = {(Mdec, sps): [receive(o, wire, WIRE_FREQS[c], cd, Mdec, sps, pattern, WIRE_SHIFT) for c in range(C_)]
          for Mdec, sps in RECEIVERS}
    _CHAIN["wire", seed] = dict(bits=bits, pre=pre, pay=pay, pattern=pattern, total=total, wire=wire, rx=rx)
    return _CHAIN["wire", seed]


def payload_of(r, sps):
    """The decoded payload: D outputs dropped, then one per symbol."""
    return r["bits"][sps::sps], r["soft"][sps::sps]


def test_oracle_link_chain_decodes_every_burst(O):
    r = link_chain(O["strict"])
    for c in range(C_):
        row = r["rows"][c]
        found, idx = row["hit"]
        assert found, c
        assert idx == OFFS[c] + NPRE - 1 + DELAY, (c, idx)  # the preamble's last symbol, later by the filters' delay
        got, soft = payload_of(row, 1)
        assert len(got) == NPAY and int((got != r["pay"][c]).sum()) == 0, c  # a condition, not a tolerance
        # every bit of the row from the second onward is the bit sent 8 symbols earlier, idle bits included
        sent = (r["bits"][c] > 0).astype(np.uint8)
        assert np.array_equal(row["whole"][DELAY + 1:], sent[1:NBITS - DELAY]), c
        assert 7.0e6 < row["tq"].min() and row["tq"].max() < 4.0e7, (c, row["tq"].min(), row["tq"].max())
        assert 14 <= np.abs(soft.astype(np.int32)).min() and np.abs(soft.astype(np.int32)).max() < 127, c


def test_oracle_wire_chain_decodes_every_burst_in_both_receivers(O):
    r = wire_chain(O["strict"])
    # the composite does not saturate after the shift (before it, it would: shift 0 clips)
    peak = int(np.abs(r["total"]).max())
    assert 32767 < peak < 32767 << COMBINE_SHIFT, peak
    assert np.array_equal(r["wire"].astype(np.int64), r["total"] >> COMBINE_SHIFT)
    for Mdec, sps in RECEIVERS:
        for c in range(C_):
            row = r["rx"][Mdec, sps][c]
            found, idx = row["hit"]
            assert found, (Mdec, c)
            assert idx == sps * (OFFS[c] + NPRE - 1 + DELAY), (Mdec, c, idx)
            got, soft = payload_of(row, sps)
            assert len(got) == NPAY and int((got != r["pay"][c]).sum()) == 0, (Mdec, c)
            assert 2.0e6 < row["tq"].min() and row["tq"].max() < 1.2e7, (Mdec, c, row["tq"].min(), row["tq"].max())
            assert 20 <= np.abs(soft.astype(np.int32)).min() and np.abs(soft.astype(np.int32)).max() < 127, (Mdec, c)


def gpu_receive(S, x, freqs, cd, Mdec, sps, pattern, shift, want, pay):
    """The DDC bank, the correlator bank and the SDPSK bank over x ([C, n, 2],
    or [n, 2] shared) against the oracle chain's rows."""
    import torch
    rxm, decims, cors = [], [], []
    for c in range(C_):
        m = S.Mixer(4096)
        m.reset(-freqs[c])
        rxm.append(m)
        decims.append(S.FilterDnsamplingFir(cd, Mdec, *I16))
        g = S.FixedPatternCorrelator(NPRE, sps)
        g.setPattern(pattern)
        cors.append(g)
    base = torch.zeros((C_, x.shape[-2] // Mdec, 2), dtype=torch.int16, device="cuda")
    S.mixdecim_step_batched(rxm, decims, x, base)
    got = S.corr_step_batched(cors, base)
    assert got == [w["hit"] for w in want] and all(f for f, _ in got)
    y = base.cpu().numpy()
    for c in range(C_):
        assert np.array_equal(y[c], want[c]["base"]), c
    demods = [S.DemodulatorSdpsk(sps, shift) for _ in range(C_)]
    n = sps * NPAY + sps
    soft, bits = S.sdpsk_step_batched(demods, base, offsets=[idx for _, idx in got], n=n)  # D samples early
    soft, bits = soft.cpu().numpy(), bits.cpu().numpy()
    for c in range(C_):
        assert np.array_equal(soft[c], want[c]["soft"]) and np.array_equal(bits[c], want[c]["bits"]), c
        D, sh, carry = demods[c].state()
        assert (D, sh) == (sps, shift) and np.array_equal(carry, want[c]["carry"]), c
        assert np.array_equal(bits[c, sps::sps], pay[c]), c  # every payload bit


@pytest.mark.gpu
def test_gpu_link_chain_equals_the_oracle_chain(S, O):
    import torch
    r = link_chain(O["strict"])
    cu, cd = link_filters()
    maps = [S.SymbolMapperSdpsk() for _ in range(C_)]
    ups = [S.FilterUpsamplingFir(cu, L_LINK, *I16) for _ in range(C_)]
    tx = []
    for c in range(C_):
        m = S.Mixer(4096)
        m.reset(FREQS[c])
        tx.append(m)
    carrier = torch.zeros((C_, L_LINK * NBITS, 2), dtype=torch.int16, device="cuda")
    S.modulate_step_batched(maps, ups, tx, torch.from_numpy(r["bits"]).cuda(), carrier)
    gpu_receive(S, carrier, FREQS, cd, L_LINK, 1, r["pattern"], LINK_SHIFT, r["rows"], r["pay"])


@pytest.mark.gpu
def test_gpu_wire_chain_equals_the_oracle_chain(S, O):
    import torch
    r = wire_chain(O["strict"])
    cu, cd = wire_filters()
    maps = [S.SymbolMapperSdpsk() for _ in range(C_)]
    ups = [S.FilterUpsamplingFir(cu, WIRE_L, *I16) for _ in range(C_)]
    tx = []
    for c in range(C_):
        m = S.Mixer(4096)
        m.reset(WIRE_FREQS[c])
        tx.append(m)
    carriers = torch.zeros((C_, WIRE_L * NBITS, 2), dtype=torch.int16, device="cuda")
    wire = torch.zeros((WIRE_L * NBITS, 2), dtype=torch.int16, device="cuda")  # ONE row
    S.modulate_step_batched(maps, ups, tx, torch.from_numpy(r["bits"]).cuda(), carriers)
    assert S.combine(carriers, wire, COMBINE_SHIFT) is wire
    assert np.array_equal(wire.cpu().numpy(), r["wire"])
    for Mdec, sps in RECEIVERS:  # the composite as the shared input of both receivers
        gpu_receive(S, wire, WIRE_FREQS, cd, Mdec, sps, r["pattern"], WIRE_SHIFT, r["rx"][Mdec, sps], r["pay"])
