"""One carrier with three offset-QPSK bursts in one row, through the chain of
test_gpu_oqpsk_loop.py (its filters, preamble, pattern and rates): modulator
-> DDC -> every detection of the row in one stepAll -> one demodulator per
detection.  The oracle and model chain here is what the GPU test must equal.

The idle bits between the bursts are random and a correlator at its default
threshold may fire on them, or again two samples after a burst's detection:
through the oracle chain the idle-bit seed 3001 gives such extra detections
(as 3003 .. 3005 do), 3002 gives the three bursts alone.  The seed is chosen
from the oracle chain only."""
import numpy as np

import corr_all_model as CM
import demod_model as DM
import mapper_model as M
import stagger_model as G
import test_gpu_oqpsk_loop as Q

NBITS, OFFS, FREQ, SEED = 2400, (40, 433, 820), 0.11, 3002


def build(seed=SEED):
    rng = np.random.default_rng(seed)
    pre = np.random.default_rng(5).integers(0, 2, Q.NPRE).astype(np.uint8)  # the preamble of test_gpu_oqpsk_loop
    bits = rng.choice(np.array([0, 1, 255], np.uint8), NBITS)
    pay = np.zeros((3, Q.NPAY), np.uint8)
    for k, off in enumerate(OFFS):
        pay[k] = rng.integers(0, 2, Q.NPAY)
        bits[2 * off:2 * off + Q.NPRE + Q.NPAY] = np.concatenate([pre, pay[k]])
    s = DM.oqpsk_samples(pre, 1.0).astype(np.float64)
    pattern = np.round(s * (24324.0 / np.sqrt((s * s).sum()))).astype(np.int32)
    return bits, pre, pay, pattern


def oracle_chain(o, seed=SEED):
    bits, pre, pay, pattern = build(seed)
    cu, cd = Q.filters()
    tx_m, rx_m = o.mixer(4096), o.mixer(4096)
    tx_m.reset(FREQ)
    rx_m.reset(-FREQ)
    y = np.asarray(o.up(0, Q.L, cu).step(M.MapperModel(M.QPSK).step(bits))).reshape(-1, 2)
    carrier = tx_m.step(G.StaggerModel(Q.D).step(y))
    base = np.asarray(o.decim(1, Q.MDEC, cd).step(rx_m.step(carrier))).reshape(-1, 2)
    corr = o.corr(Q.NPRE, 1)
    corr.set_pattern(pattern)
    idx, rows, used = CM.step_all(corr, base, 16)
    refs, soft, errs = [], [], []
    for i, row in zip(idx.tolist(), rows):
        ref = Q.remove_modulation(row, pattern)
        m = DM.DemodModel()
        m.set_sync_pattern(pre)
        m.set_reference(ref)
        m.set_initial_frequency(0.0)
        m.reset()
        first = i - (Q.NPRE - 1)
        sb, e = m.step(base[first:first + Q.NPRE + Q.NPAY])
        refs.append(ref)
        soft.append(sb)
        errs.append(e)
    return bits, pre, pay, pattern, idx.tolist(), base, refs, soft, errs
