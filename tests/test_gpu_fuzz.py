"""Seeded differential fuzzing of the HIP path against the C oracle (which
tests/test_oracle_golden.py pins to the reference): random operator shapes,
random chains of step() calls of ragged lengths (including 0 and 1), resets,
left shifts and coefficient changes, device-resident and host-staged calls
interleaved.  Every output byte must match.  Shapes are drawn to hit the tuned
kernels (63/64/127/128/255/256 taps at M = 1/2/3/4/8/16, M = 1, L = 2/4 with 16/32/64
taps per phase) as often as the generic ones.

The transmit operators (srcdsp_upmix_*, srcdsp_mapper_*, srcdsp_stagger_*,
srcdsp_modulate_*, srcdsp_modulate_offset_*) are fuzzed as chains against
tests/tx_chain_model.py, the composition of the mapper model, the oracle's
interpolator and mixer and the stagger model that tests/test_tx_chain_model.py
holds to the reference's goldens: ragged steps, flushes in mid-stream, the
iterator form, retunes, resets, copies, the fused call and the separate
operators taking turns on the same handles, inputs off 16-byte alignment, and
banks of 1 to 65 rows at any strides; after every call every output byte and
every state, the guard band behind every row, and the path counter the
documented dispatch rule predicts.  The draws are tests/tx_fuzz_draw.py's.

The rational resampler (srcdsp_resample_*) is fuzzed the same way against the
oracle's interpolator and decimator in sequence, under
resample_set_min_tiles(1): L, M, taps per phase and decimator taps on and off
what the fused kernel takes, legal ragged steps, flushes, the fused call and
the two single operators taking turns on the same handles, inputs off 16-byte
alignment, new left shifts, resets, copies, and banks of 1 to 65 rows at any
strides; after every call every output sample, the decimator's state, the
interpolator's next call on a copy, the guard band and the path counter the
dispatch rule predicts.  The draws are tests/resample_fuzz_draw.py's
(tests/test_resample_fuzz_draw.py holds them to their conditions)."""
import numpy as np
import pytest

import resample_fuzz_draw as R
import tx_fuzz_draw as F
from tx_chain_model import UPMIX, TxChain

pytestmark = pytest.mark.gpu

_DECIM_T = {0: ("complex<float>", "complex<float>", "complex<float>", "float"),
            1: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t"),
            2: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int16_t"),
            3: ("complex<int32_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")}
_FIR_T = {0: ("complex<float>", "complex<float>", "complex<float>", "float"),
          1: ("float", "complex<float>", "float", "float"),
          2: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")}
_UP_T = {0: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t"),
         1: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int16_t"),
         2: ("int16_t", "int16_t", "int32_t", "int32_t")}


@pytest.fixture(scope="module")
def O():
    import pyoracle
    return {"strict": pyoracle.Oracle(0), "fma": pyoracle.Oracle(1)}


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(op, x, on_device):
    if on_device:
        return op.step(_dev(x)).cpu().numpy()
    return op.step(x)


def _taps(rng, variant, n):
    if variant == 0:
        return (rng.standard_normal(n) / max(2.0, n / 4)).astype(np.float32)
    if variant == 2:
        return rng.integers(-2000, 2000, n).astype(np.int16)
    kind = rng.integers(0, 3)  # int16 range (dot2), < 2^23 (mad24), wide
    lim = (32767, (1 << 23) - 1, 1 << 26)[kind]
    return rng.integers(-lim, lim + 1, n).astype(np.int32)


def _input(rng, O, variant, n):
    if variant == 0:
        x = O["fma"].gen_cf32(int(rng.integers(1 << 30)), 0, 0, n, -30000, 30000)
        if n and rng.random() < 0.2:  # a few large / special values
            k = rng.integers(0, n, 3)
            x[k] = np.array([3e9 + 1j, -np.inf + 0j, np.nan * 1j], np.complex64)[: len(k)]
        return x
    if variant == 3:
        return rng.integers(-(1 << 20), 1 << 20, size=(n, 2)).astype(np.int32)
    return O["fma"].gen_ci16(int(rng.integers(1 << 30)), 0, 0, n, -32768, 32767)


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_decimator(S, O, seed):
    rng = np.random.default_rng(1000 + seed)
    variant = int(rng.integers(0, 4))
    M = int(rng.choice([1, 2, 3, 4, 4, 4, 5, 8, 16]))
    ntaps = int(rng.choice([1, 2, 7, 31, 63, 64, 127, 127, 128, 129, 200, 255, 256]))
    fp = str(rng.choice(["fma", "strict"]))
    c = _taps(rng, variant, ntaps)
    g = S.FilterDnsamplingFir(c, M, *_DECIM_T[variant], fp=fp)
    r = O[fp].decim(variant, M, c)
    for op in range(10):
        u = rng.random()
        if u < 0.08:
            g.reset()
            r.reset()
        elif u < 0.14:
            ls = int(rng.integers(0, 3))
            g.setLeftShiftBy2(ls)
            r.set_left_shift(ls)
        elif u < 0.2:
            c = _taps(rng, variant, int(rng.choice([ntaps, 1, 63, 64, 127, 128, 255])))
            g.setCoeffs(c, require_multiple=False)
            r.set_coeffs(c)
        n = M * int(rng.choice([0, 1, 3, 17, 1024, 4099, 20000, int(rng.integers(0, 30000))]))
        x = _input(rng, O, variant, n)
        got, exp = _run(g, x, bool(rng.integers(0, 2))), r.step(x)
        assert got.tobytes() == exp.tobytes(), (seed, op, variant, M, ntaps, fp, n)


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_fir(S, O, seed):
    rng = np.random.default_rng(2000 + seed)
    variant = int(rng.integers(0, 3))
    ntaps = int(rng.choice([1, 3, 31, 31, 100, 128, 129, 500, 1100]))
    fp = str(rng.choice(["fma", "strict"]))
    tv = {0: 0, 1: 0, 2: 1}[variant]
    c = _taps(rng, tv, ntaps).astype(np.float32 if variant < 2 else np.int32)
    g = S.FilterFir(c, *_FIR_T[variant], fp=fp)
    r = O[fp].fir(variant, c)
    for op in range(8):
        if rng.random() < 0.1:
            g.reset()
            r.reset()
        n = int(rng.choice([0, 1, 5, 2048, 2049, 9000, int(rng.integers(0, 20000))]))
        if variant == 1:
            x = O["fma"].gen_cf32(int(rng.integers(1 << 30)), 0, 0, n, -30000, 30000).real.astype(np.float32)
        else:
            x = _input(rng, O, 0 if variant == 0 else 1, n)
        got, exp = _run(g, x, bool(rng.integers(0, 2))), r.step(x)
        assert got.tobytes() == exp.tobytes(), (seed, op, variant, ntaps, fp, n)


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_upsampler(S, O, seed):
    rng = np.random.default_rng(3000 + seed)
    variant = int(rng.integers(0, 3))
    L = int(rng.choice([1, 2, 3, 4, 4, 8]))
    H = int(rng.choice([1, 2, 5, 16, 32, 33, 64, 70]))
    lim = {0: int(rng.choice([32767, 1 << 22, 1 << 26])), 1: 32767, 2: 30000}[variant]
    c = rng.integers(-lim, lim + 1, L * H)
    g = S.FilterUpsamplingFir(c, L, *_UP_T[variant])
    r = O["fma"].up(variant, L, c)
    for op in range(8):
        if rng.random() < 0.1:
            g.reset()
            r.reset()
        n = int(rng.choice([0, 1, 7, 2048, 2049, int(rng.integers(0, 9000))]))
        x = O["fma"].gen_ci16(int(rng.integers(1 << 30)), 0, 0, n, -32768, 32767)
        if variant == 2:
            x = np.ascontiguousarray(x[:, 0])
        flush, it = bool(rng.random() < 0.2), bool(rng.random() < 0.3)
        if bool(rng.integers(0, 2)):
            got = g.step(_dev(x), None, flush, it).cpu().numpy()
        else:
            got = g.step(x, None, flush, it)
        exp = r.step(x, flush, it)
        assert got.tobytes() == exp.tobytes(), (seed, op, variant, L, H, n, flush, it)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_mixer_and_chain(S, O, seed):
    rng = np.random.default_rng(4000 + seed)
    N = int(rng.choice([16, 1000, 4096, 4096]))
    f = float(rng.uniform(-1, 1))
    m, om = S.Mixer(N), O["fma"].mixer(N)
    m.reset(f)
    om.reset(f)
    fused = bool(rng.integers(0, 2))
    if fused:
        from srcdsp_amd.design import hamming_sinc, q14
        # M = 4 x 127/128 is the fused kernel; the others run as the two calls
        Md = int(rng.choice([4, 4, 4, 2, 8]))
        cq = q14(hamming_sinc(int(rng.choice([127, 128, 63])), 0.12))
        d = S.FilterDnsamplingFir(cq, Md, *_DECIM_T[1])
        chain = S.MixerDecimatorChain(m, d)
        od = O["fma"].decim(1, Md, cq)
    for op in range(8):
        u = rng.random()
        if u < 0.15:
            a = float(rng.uniform(-0.5, 0.5))
            m.adjustFrequency(a)
            om.adjust_frequency(a)
        elif u < 0.25:
            f = float(rng.uniform(-1, 1))
            m.setFrequency(f)
            om.set_frequency(f)
        n = 8 * int(rng.choice([0, 1, 7, 1000, 4097, int(rng.integers(0, 20000))]))
        x = O["fma"].gen_ci16(int(rng.integers(1 << 30)), 0, 0, n, -32768, 32767)
        if fused:
            got = chain.step(_dev(x)).cpu().numpy()
            exp = od.step(om.step(x))
        else:
            got = _run(m, x, bool(rng.integers(0, 2)))
            exp = om.step(x)
        assert got.tobytes() == exp.tobytes(), (seed, op, N, fused, n)
        assert m.state()[:2] == om.state()[:2]


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_correlator(S, O, seed):
    from srcdsp_amd.design import qpsk_pattern
    rng = np.random.default_rng(5000 + seed)
    N, Sx = [(32, 1), (32, 4), (64, 2), (1024, 1), (48, 1), (16, 3)][seed % 6]
    p = qpsk_pattern(N, int(rng.choice([200, 500])), seed=seed)
    g, r = S.FixedPatternCorrelator(N, Sx), O["fma"].corr(N, Sx)
    g.setPattern(p)
    r.set_pattern(p)
    for op in range(6):
        if rng.random() < 0.1:
            g.reset()
            r.reset()
        n = int(rng.choice([0, 1, 5, 5000, 30000, int(rng.integers(0, 40000))]))
        x = rng.integers(-125, 126, size=(n, 2))
        for _ in range(int(rng.integers(0, 3))):  # embedded copies of the pattern (strided by S)
            if n > N * Sx + 10:
                at = int(rng.integers(0, n - N * Sx))
                x[at:at + N * Sx:Sx] += 2 * p
        x = np.clip(x, -32768, 32767).astype(np.int16)
        got = g.step(_dev(x)) if bool(rng.integers(0, 2)) else g.step(x)
        exp = r.step(x)
        assert got[0] == exp[0] and (not exp[0] or got[1] == exp[1]), (seed, op, N, Sx, n, got, exp)
        if exp[0]:
            assert np.array_equal(g.getRefBitSamples(), r.bit_samples())
        st = r.status()
        gs = g.getStatus()
        assert list(gs["corr"]) == st["corr"] and list(gs["energy"]) == st["energy"], (seed, op)


# --- the run-time-shape kernels of round 3, drawn over their whole ranges ---
# (decim_stream_cf32 / decim_dot2_ci16 at any N <= 1024 and M in {1, 2, 3, 4,
# 6, 8, 12, 16}; up_tile_dot2 at L = 2..8 and any taps per phase;
# corr_eval_dot2 at any N >= 48 and stride S; the fused chain at any N)

def _any_taps(rng):
    return int(rng.choice([int(rng.integers(2, 48)), int(rng.integers(48, 400)), int(rng.integers(400, 1025)),
                           int(rng.integers(1025, 1300))]))


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_decimator_any_shape(S, O, seed):
    rng = np.random.default_rng(6000 + seed)
    variant = int(rng.choice([0, 0, 1, 1, 2]))
    M = int(rng.choice([1, 2, 3, 4, 6, 8, 12, 16]))
    ntaps = _any_taps(rng)
    fp = str(rng.choice(["fma", "strict"]))
    c = _taps(rng, variant, ntaps)
    if variant == 1 and rng.random() < 0.6:  # int16-range taps in an int32 filter: the dot2 kernel
        c = rng.integers(-32768, 32768, ntaps).astype(np.int32)
    g = S.FilterDnsamplingFir(c, M, *_DECIM_T[variant], fp=fp)
    r = O[fp].decim(variant, M, c)
    for op in range(6):
        if rng.random() < 0.1:
            g.reset()
            r.reset()
        n = M * int(rng.choice([0, 1, 5, 2047, 8193, int(rng.integers(0, 24000))]))
        x = _input(rng, O, variant, n)
        got, exp = _run(g, x, bool(rng.integers(0, 2))), r.step(x)
        assert got.tobytes() == exp.tobytes(), (seed, op, variant, M, ntaps, fp, n)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_upsampler_any_shape(S, O, seed):
    rng = np.random.default_rng(7000 + seed)
    L = int(rng.integers(2, 9))
    H = int(rng.choice([int(rng.integers(1, 20)), int(rng.integers(20, 140))]))
    c = rng.integers(-32767, 32768, L * H)
    g = S.FilterUpsamplingFir(c, L, *_UP_T[0])
    r = O["fma"].up(0, L, c)
    for op in range(6):
        if rng.random() < 0.1:
            g.reset()
            r.reset()
        n = int(rng.choice([0, 1, 7, 2048, 4099, int(rng.integers(0, 12000))]))
        x = O["fma"].gen_ci16(int(rng.integers(1 << 30)), 0, 0, n, -32768, 32767)
        flush, it = bool(rng.random() < 0.2), bool(rng.random() < 0.3)
        if bool(rng.integers(0, 2)):
            got = g.step(_dev(x), None, flush, it).cpu().numpy()
        else:
            got = g.step(x, None, flush, it)
        exp = r.step(x, flush, it)
        assert got.tobytes() == exp.tobytes(), (seed, op, L, H, n, flush, it)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_correlator_any_shape(S, O, seed):
    from srcdsp_amd.design import qpsk_pattern
    rng = np.random.default_rng(8000 + seed)
    N, Sx = int(rng.integers(48, 330)), int(rng.integers(1, 6))
    p = qpsk_pattern(N, int(rng.choice([200, 500])), seed=seed)
    g, r = S.FixedPatternCorrelator(N, Sx), O["fma"].corr(N, Sx)
    g.setPattern(p)
    r.set_pattern(p)
    for op in range(5):
        if rng.random() < 0.1:
            g.reset()
            r.reset()
        n = int(rng.choice([0, 1, 5, 9000, int(rng.integers(0, 40000))]))
        x = rng.integers(-125, 126, size=(n, 2))
        for _ in range(int(rng.integers(0, 3))):
            if n > N * Sx + 10:
                at = int(rng.integers(0, n - N * Sx))
                x[at:at + N * Sx:Sx] += 2 * p
        x = np.clip(x, -32768, 32767).astype(np.int16)
        got = g.step(_dev(x)) if bool(rng.integers(0, 2)) else g.step(x)
        exp = r.step(x)
        assert got[0] == exp[0] and (not exp[0] or got[1] == exp[1]), (seed, op, N, Sx, n, got, exp)
        if exp[0]:
            assert np.array_equal(g.getRefBitSamples(), r.bit_samples())
        st, gs = r.status(), g.getStatus()
        assert list(gs["corr"]) == st["corr"] and list(gs["energy"]) == st["energy"], (seed, op, N, Sx)


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_chain_any_shape(S, O, seed):
    rng = np.random.default_rng(9000 + seed)
    N = int(rng.choice([16, 1000, 4096]))
    f = float(rng.uniform(-1, 1))
    m, om = S.Mixer(N), O["fma"].mixer(N)
    m.reset(f)
    om.reset(f)
    Md = int(rng.choice([1, 2, 4, 8, 16]))
    nt = int(rng.integers(2, 1025))
    c = rng.integers(-32768, 32768, nt).astype(np.int32)
    d = S.FilterDnsamplingFir(c, Md, *_DECIM_T[1])
    chain = S.MixerDecimatorChain(m, d)
    od = O["fma"].decim(1, Md, c)
    for op in range(6):
        if rng.random() < 0.15:
            a = float(rng.uniform(-0.5, 0.5))
            m.adjustFrequency(a)
            om.adjust_frequency(a)
        n = 16 * int(rng.choice([0, 1, 7, 1000, int(rng.integers(0, 12000))]))
        x = O["fma"].gen_ci16(int(rng.integers(1 << 30)), 0, 0, n, -32768, 32767)
        got = chain.step(_dev(x)).cpu().numpy()
        exp = od.step(om.step(x))
        assert got.tobytes() == exp.tobytes(), (seed, op, N, Md, nt, n)
        assert m.state()[:2] == om.state()[:2]


# --- the transmit chains: every fused family, single calls and banks ---

def _tx_pair(S, O, sh, freq=None, state=None):
    from tx_gpu import GpuChain
    freq = sh["freq"] if freq is None else freq
    state = sh["mapper_state"] if state is None else state
    args = (sh["family"], sh["L"], sh["taps"], sh["N"], freq)
    kw = dict(kind=sh["kind"], D=sh["D"], variant=sh["variant"], mapper_state=state)
    return GpuChain(S, *args, **kw), TxChain(O["strict"], *args, **kw)


def _one_hot(i):
    return tuple(int(k == i) for k in range(4))


@pytest.mark.parametrize("seed", range(F.CHAIN_SEEDS))
def test_fuzz_transmit_chain(S, O, seed):
    from tx_gpu import GUARD_VALUE, dev, dev_off
    rng = F.chain_rng(seed)
    sh = F.draw_shape(rng)
    ops = F.draw_ops(rng, sh)
    g, m = _tx_pair(S, O, sh)
    what = (seed, sh["family"], sh["kind"], sh["L"], sh["H"], sh["variant"], sh["taps_kind"], sh["N"], sh["D"])
    for k, op in enumerate(ops):
        if op[0] == "copy":  # go on with copies of all handles
            g, m = g.copy(), m.copy()
            continue
        if op[0] != "step":
            getattr(g, op[0])(*op[1:])
            getattr(m, op[0])(*op[1:])
            continue
        a = op[1]
        x = F.draw_input(rng, sh, a["n"])
        xd = dev_off(x) if a["off"] else dev(x)
        exp = m.step(x, a["flush"], a["iterator"])
        s0 = g.stats()
        if a["fused"]:
            buf = g.guarded(len(exp))
            g.fused(xd, a["flush"], a["iterator"], buf[:len(exp)])
            got = buf.cpu().numpy()
            assert (got[len(exp):] == GUARD_VALUE).all(), (what, k, a)
            got = got[:len(exp)]
        else:
            got = g.separate(xd, a["flush"], a["iterator"]).cpu().numpy()
        rose = tuple(b - c for c, b in zip(s0, g.stats()))
        if not a["fused"] or len(exp) == 0:
            assert rose == (0, 0, 0, 0), (what, k, a, rose)
        else:  # the fused kernel where the dispatch rule says so, else the pair / sequence
            assert rose == _one_hot(0 if F.eligible(sh) and not a["off"] else 1), (what, k, a, rose)
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), (what, k, a)
        assert g.state() == m.state(), (what, k, a)


@pytest.mark.parametrize("seed", range(F.BANK_SEEDS))
def test_fuzz_transmit_bank(S, O, seed):
    import torch
    from tx_gpu import GUARD, GUARD_VALUE, bank_step, dev
    rng = F.bank_rng(seed)
    sh = F.draw_bank(rng)
    rows, samples = sh["rows"], sh["family"] == UPMIX
    what = (seed, sh["family"], sh["kind"], sh["L"], sh["H"], sh["variant"], sh["taps_kind"], sh["N"], sh["D"], rows,
            sh["shared"])
    ps = []
    for r in range(rows):  # every row its own carrier, mapper state, history and carry
        g, m = _tx_pair(S, O, sh, float(rng.uniform(-1, 1)), int(rng.integers(0, 4)))
        x = F.draw_input(rng, sh, int(rng.integers(1, 12)))
        assert g.separate(dev(x)).cpu().numpy().tobytes() == m.step(x).tobytes(), (what, r)
        ps.append((g, m))
    chains = [g for g, _ in ps]
    unit = 4 if samples else 16  # elements in 16 bytes
    for k, (n_sym, flush) in enumerate(sh["calls"]):
        xs = [F.draw_input(rng, sh, n_sym) for _ in range(1 if sh["shared"] else rows)]
        n = len(xs[0])
        if sh["shared"]:
            in_stride, xd = 0, dev(xs[0])
        else:
            in_stride = (n + unit - 1) // unit * unit + (0 if sh["in_stride16"] else 1)
            host = np.zeros((rows, in_stride) + xs[0].shape[1:], xs[0].dtype)
            host[:, :n] = np.stack(xs)
            xd = dev(host)
        exps = [m.step(xs[0 if sh["shared"] else r], flush) for r, (_, m) in enumerate(ps)]
        n_out = len(exps[0])
        out_stride = (n_out + GUARD + 3) // 4 * 4 + (0 if sh["out_stride16"] else 1)
        out = torch.full((rows, out_stride, 2), GUARD_VALUE, dtype=torch.int16, device="cuda")
        s0 = chains[0].stats()
        bank_step(chains, xd if n else None, in_stride, out, n, flush)
        rose = tuple(b - c for c, b in zip(s0, chains[0].stats()))
        strides16 = in_stride * (4 if samples else 1) % 16 == 0 and out_stride * 4 % 16 == 0
        if n_out == 0:
            assert rose == (0, 0, 0, 0), (what, k, rose)
        else:  # one launch per 64 rows where the dispatch rule says so, else the loop over the rows
            assert rose == _one_hot(2 if F.eligible(sh) and strides16 else 3), (what, k, rose)
        got = out.cpu().numpy()
        assert (got[:, n_out:] == GUARD_VALUE).all(), (what, k)
        for r, (g, m) in enumerate(ps):
            assert got[r, :n_out].tobytes() == exps[r].tobytes(), (what, k, r)
            assert g.state() == m.state(), (what, k, r)


# --- the rational resampler: the fused interpolator -> decimator call, single and banks ---

_RS_GUARD, _RS_GUARD_VALUE = 24, 0x5A5A


class _RsModel:
    """The oracle's two calls with what fixes their state, so that a copy can
    be rebuilt: the interpolator with its last inputs (tx_chain_model._Up), the
    decimator with its left shift and the last N_d - 1 interpolated samples."""

    def __init__(self, o, sh, up=None, ls=None, tail=None):
        from tx_chain_model import _Up
        self.o, self.sh = o, sh
        self.up = _Up(o, sh["uvar"], sh["L"], sh["cu"]) if up is None else up
        self.dec = o.decim(sh["dvar"], sh["M"], sh["cd"])
        self.ls = sh["ls"] if ls is None else ls
        self.dec.set_left_shift(self.ls)
        self.tail = np.zeros((sh["Nd"] - 1, 2), np.int16)
        if tail is not None and len(tail):  # whole blocks of M ending in the tail: the outputs are dropped
            self.dec.step(np.concatenate([np.zeros(((-len(tail)) % sh["M"], 2), np.int16), tail]))
            self.tail = tail.copy()

    def copy(self):
        return _RsModel(self.o, self.sh, self.up.copy(), self.ls, self.tail)

    def set_left_shift(self, ls):
        self.ls = ls
        self.dec.set_left_shift(ls)

    def reset_up(self):
        self.up.reset()

    def reset_decim(self):
        self.dec.reset()
        self.tail[:] = 0

    def step(self, x, flush=False):
        mid = self.up.step(x, flush, False)
        fed = np.concatenate([self.tail, mid])
        self.tail = fed[len(fed) - (self.sh["Nd"] - 1):].copy()
        return self.dec.step(mid)

    def same_decim_state(self, dec, what):
        """As the handle reports it."""
        st = dec.state()
        assert st["coeff_scaling"] == self.dec.coeff_scaling and st["left_shift"] == self.ls, what
        assert st["history"].tobytes() == self.tail.tobytes(), what

    def same_up_state(self, up, probe, what):
        """The interpolator's history, as a further step of copies shows it."""
        import copy
        got = copy.copy(up).step(_dev(probe)).cpu().numpy()
        assert got.tobytes() == self.up.copy().step(probe, False, False).tobytes(), what


class _RsGpu:
    def __init__(self, S, sh):
        cu = sh["cu"].astype(np.int16) if sh["uvar"] == 1 else sh["cu"]
        cd = sh["cd"].astype(np.int16) if sh["dvar"] == 2 else sh["cd"]
        self.up = S.FilterUpsamplingFir(cu, sh["L"], *_UP_T[sh["uvar"]])
        self.dec = S.FilterDnsamplingFir(cd, sh["M"], *_DECIM_T[sh["dvar"]])
        self.dec.set_left_shift(sh["ls"])

    def copy(self):
        import copy
        c = object.__new__(_RsGpu)
        c.up, c.dec = copy.copy(self.up), copy.copy(self.dec)
        return c

    def set_left_shift(self, ls):
        self.dec.set_left_shift(ls)

    def reset_up(self):
        self.up.reset()

    def reset_decim(self):
        self.dec.reset()


@pytest.fixture
def resample_every_tile_count(S):
    """The fused resampler kernel serves whatever it takes, however short."""
    S.resample_set_min_tiles(1)
    yield
    S.resample_set_min_tiles(0)


def _rs_what(seed, sh):
    return (seed, sh["L"], sh["H"], sh["M"], sh["Nd"], sh["uvar"], sh["dvar"], sh["taps_kind"])


@pytest.mark.parametrize("seed", range(R.CHAIN_SEEDS))
def test_fuzz_resample_chain(S, O, resample_every_tile_count, seed):
    import torch
    from tx_gpu import dev, dev_off
    rng = R.chain_rng(seed)
    sh = R.draw_shape(rng)
    ops = R.draw_ops(rng, sh)
    g, m = _RsGpu(S, sh), _RsModel(O["strict"], sh)
    what = _rs_what(seed, sh)
    probe = R.draw_input(rng, 40)
    for k, op in enumerate(ops):
        if op[0] == "copy":  # go on with copies of both handles
            g, m = g.copy(), m.copy()
            continue
        if op[0] != "step":
            getattr(g, op[0])(*op[1:])
            getattr(m, op[0])(*op[1:])
            continue
        a = op[1]
        x = R.draw_input(rng, a["n"])
        xd = dev_off(x) if a["off"] else dev(x)
        exp = m.step(x, a["flush"])
        s0 = S.resample_stats()
        if a["fused"]:
            buf = torch.full((len(exp) + _RS_GUARD, 2), _RS_GUARD_VALUE, dtype=torch.int16, device="cuda")
            S.RationalResampler(g.up, g.dec).step(xd, buf[:len(exp)], a["flush"])
            got = buf.cpu().numpy()
            assert (got[len(exp):] == _RS_GUARD_VALUE).all(), (what, k, a)
            got = got[:len(exp)]
        else:
            got = g.dec.step(g.up.step(xd, None, a["flush"])).cpu().numpy()
        rose = tuple(b - c for c, b in zip(s0, S.resample_stats()))
        if not a["fused"] or len(exp) == 0:
            assert rose == (0, 0, 0, 0), (what, k, a, rose)
        else:  # the fused kernel where the dispatch rule says so, else the pair
            assert rose == _one_hot(0 if R.eligible(sh) and not a["off"] else 1), (what, k, a, rose)
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), (what, k, a)
        m.same_decim_state(g.dec, (what, k, a))
        m.same_up_state(g.up, probe, (what, k, a))


@pytest.mark.parametrize("seed", range(R.BANK_SEEDS))
def test_fuzz_resample_bank(S, O, resample_every_tile_count, seed):
    import torch
    from tx_gpu import dev
    rng = R.bank_rng(seed)
    sh = R.draw_bank(rng)
    rows = sh["rows"]
    what = _rs_what(seed, sh) + (rows,)
    ps = []
    for r in range(rows):  # every row its own histories
        g, m = _RsGpu(S, sh), _RsModel(O["strict"], sh)
        x = R.draw_input(rng, sh["g"] * int(rng.integers(1, 12)))
        assert g.dec.step(g.up.step(dev(x))).cpu().numpy().tobytes() == m.step(x).tobytes(), (what, r)
        ps.append((g, m))
    ups, decs = [g.up for g, _ in ps], [g.dec for g, _ in ps]
    probe = R.draw_input(rng, 40)
    for k, (n, flush) in enumerate(sh["calls"]):
        xs = [R.draw_input(rng, n) for _ in range(rows)]
        in_stride = max((n + 3) // 4 * 4, 4) + (0 if sh["in_stride16"] else 1)
        host = np.zeros((rows, in_stride, 2), np.int16)
        host[:, :n] = np.stack(xs)
        xd = dev(host)[:, :n]
        exps = [m.step(xs[r], flush) for r, (_, m) in enumerate(ps)]
        n_out = len(exps[0])
        out_stride = (n_out + _RS_GUARD + 3) // 4 * 4 + (0 if sh["out_stride16"] else 1)
        out = torch.full((rows, out_stride, 2), _RS_GUARD_VALUE, dtype=torch.int16, device="cuda")
        s0 = S.resample_stats()
        S.resample_step_batched(ups, decs, xd, out, flush)
        rose = tuple(b - c for c, b in zip(s0, S.resample_stats()))
        if n_out == 0:
            assert rose == (0, 0, 0, 0), (what, k, rose)
        else:  # one launch per 64 rows where the dispatch rule says so, else the loop over the rows
            assert rose == _one_hot(2 if R.bank_eligible(sh) else 3), (what, k, rose)
        got = out.cpu().numpy()
        assert (got[:, n_out:] == _RS_GUARD_VALUE).all(), (what, k)
        for r, (g, m) in enumerate(ps):
            assert got[r, :n_out].tobytes() == exps[r].tobytes(), (what, k, r)
            m.same_decim_state(g.dec, (what, k, r))
        for r in sorted({0, rows // 2, rows - 1}):  # the model's copy replays a history on the CPU: three rows
            g, m = ps[r]
            m.same_up_state(g.up, probe, (what, k, r))
