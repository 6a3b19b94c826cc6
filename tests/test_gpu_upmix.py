"""The interpolator -> mixer chain (srcdsp_upmix_step, srcdsp_upmix_step_batched).
Every comparison is bit-exact against the oracle's two calls
(upsampling_filters.h:149-233 then mixers.h:169-188), the mixer state
included; the process-wide counters prove which path served a call (fused
kernel / pair of operators, one bank launch / per-channel loop).

A tile is 2048 inputs.  The 9000-input stream is cut into calls of two tiles
and a ragged third, one lane, fewer inputs than the 31-sample history, exactly
one tile, and a flushing rest; every offset is a multiple of 4 samples, so the
device slices stay 16-byte aligned."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOTAL = 9000
CALLS = [4100, 8, 20, 2048, 2824]
FREQS = [0.1, -0.37, 0.5, 0.0]  # N = 4096: words 205 (odd), 3338, 1024, 0
UP_TYPES = {0: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t"),
            1: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int16_t"),
            2: ("int16_t", "int16_t", "int32_t", "int32_t")}


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def spans(total=TOTAL, calls=CALLS):
    assert sum(calls) == total
    off, out = 0, []
    for n in calls:
        out.append((off, n, off + n == total))
        off += n
    return out


def make_taps(kind, L, ntaps):
    """"sinc": a Q14 interpolation low-pass with moderate input, nothing clamps
    (about 5 % at L = 8): a wrong phase or tap order shows in every sample.
    "full": random full-range int16 taps with full-scale input: most
    interpolator outputs and about 40 % of the mixer's sit on a clamp and the
    int32 accumulators wrap, so both clamps and their order are pinned."""
    if kind == "sinc":
        from srcdsp_amd.design import hamming_sinc, q14
        return q14(hamming_sinc(ntaps, 0.48 / L) * L)
    c = np.random.default_rng(1000 * L + ntaps).integers(-32768, 32768, size=ntaps).astype(np.int32)
    c[0], c[-1] = -32768, 32767
    return c


_X, _UPREF = {}, {}


def signal(O, kind, ch=0, n=TOTAL):
    k = (kind, ch, n)
    if k not in _X:
        lo, hi = (-8192, 8191) if kind == "sinc" else (-32768, 32767)
        _X[k] = O["strict"].gen_ci16(0x0A17, ch, 0, n, lo, hi)
    return _X[k]


def up_reference(O, kind, L, ntaps, it=False, ch=0):
    """The oracle interpolator's output of every call, computed once per
    shape and shared by the mixers at every frequency and N."""
    k = (kind, L, ntaps, it, ch)
    if k not in _UPREF:
        c = make_taps(kind, L, ntaps)
        r = O["strict"].up(0, L, c // 8 if it else c)
        x = signal(O, kind, ch)
        _UPREF[k] = [r.step(x[off:off + n], last, it) for off, n, last in spans()]
    return _UPREF[k]


def mix_reference(O, ups, N, f):
    m = O["strict"].mixer(N)
    m.reset(f)
    outs, states = [], []
    for u in ups:
        outs.append(m.step(u))
        states.append(m.state()[:2])
    return outs, states


def chain(S, c, L, N, f, variant=0):
    up = S.FilterUpsamplingFir(c, L, *UP_TYPES[variant])
    m = S.Mixer(N)
    m.reset(f)
    return S.UpsamplerMixerChain(up, m)


def run_and_check(S, ch, xd, ref, it, want):
    """Step the chain over the calls; after each: outputs, mixer state and
    which counter rose (want: index into upmix_stats())."""
    outs, states = ref
    for k, (off, n, last) in enumerate(spans()):
        s0 = S.upmix_stats()
        y = ch.step(xd[off:off + n], None, last, it)
        s1 = S.upmix_stats()
        assert np.array_equal(y.cpu().numpy(), outs[k]), k
        assert ch.mixer.state()[:2] == states[k], k
        assert tuple(b - a for a, b in zip(s0, s1)) == tuple(int(i == want) for i in range(4)), k


# ------------------------------------------------------ 1. fused path
# (4,128) (2,64) (8,128): pairs per phase compiled in; (3,96) (4,100) (5,40): run-time
SHAPES = [(4, 128, 4096), (2, 64, 4096), (8, 128, 4096), (3, 96, 4096), (4, 100, 4096), (5, 40, 4096),
          (4, 128, 1024), (4, 128, 1000)]


@pytest.mark.parametrize("kind", ["sinc", "full"])
@pytest.mark.parametrize("L,ntaps,N", SHAPES)
def test_fused_kernel_vs_oracle(S, O, L, ntaps, N, kind):
    c = make_taps(kind, L, ntaps)
    xd = dev(signal(O, kind))
    ups = up_reference(O, kind, L, ntaps)
    for f in FREQS:
        run_and_check(S, chain(S, c, L, N, f), xd, mix_reference(O, ups, N, f), False, 0)


def test_fused_kernel_iterator_overload(S, O):
    """The iterator overload's shift 0, with taps // 8 as test_upsampler_vs_oracle."""
    c = make_taps("sinc", 4, 128) // 8
    xd = dev(signal(O, "sinc"))
    ups = up_reference(O, "sinc", 4, 128, it=True)
    for f in FREQS:
        run_and_check(S, chain(S, c, 4, 4096, f), xd, mix_reference(O, ups, 4096, f), True, 0)


# ------------------------------------------------------ 2. state hand-over
@pytest.mark.parametrize("fused_first", [True, False])
def test_state_hands_over_between_chain_and_single_operators(S, O, fused_first):
    L, ntaps, N, f = 4, 128, 4096, 0.1
    xd = dev(signal(O, "full"))
    outs, states = mix_reference(O, up_reference(O, "full", L, ntaps), N, f)
    ch = chain(S, make_taps("full", L, ntaps), L, N, f)
    order = [fused_first, fused_first, not fused_first, fused_first, not fused_first]
    for k, (off, n, last) in enumerate(spans()):
        xs = xd[off:off + n]
        y = ch.step(xs, None, last) if order[k] else ch.mixer.step(ch.up.step(xs, None, last))
        assert np.array_equal(y.cpu().numpy(), outs[k]), k
        assert ch.mixer.state()[:2] == states[k], k


# ------------------------------------------------------ 3. pair path
@pytest.mark.parametrize("case", ["variant1", "wide_tap", "N8192", "in_offset"])
def test_other_shapes_take_the_pair_and_stay_exact(S, O, case):
    L, ntaps, f = 4, 128, -0.37
    N = 8192 if case == "N8192" else 4096
    variant = 1 if case == "variant1" else 0
    c = make_taps("full", L, ntaps)
    if case == "wide_tap":  # beyond int16: not the dot2 tap pairs
        c = c.copy()
        c[5] = 1 << 20
    if variant == 1:
        c = c.astype(np.int16)
    ioff = 1 if case == "in_offset" else 0  # a view 4 bytes off 16-byte alignment
    x = signal(O, "full", 0, TOTAL + 4)
    xd = dev(x)[ioff:ioff + TOTAL]
    r = O["strict"].up(variant, L, c)
    ups = [r.step(x[ioff + off:ioff + off + n], last) for off, n, last in spans()]
    run_and_check(S, chain(S, c, L, N, f, variant), xd, mix_reference(O, ups, N, f), False, 1)


# ------------------------------------------------------ 4. refusals
def test_refusals_change_no_state(S, O):
    import torch
    from srcdsp_amd._capi import ERR_SIZE, ERR_UNSUPPORTED
    L, ntaps, N, f = 4, 128, 4096, 0.1
    x = signal(O, "full")
    xd = dev(x)
    outs, states = mix_reference(O, up_reference(O, "full", L, ntaps), N, f)
    ch = chain(S, make_taps("full", L, ntaps), L, N, f)
    sp = spans()
    for k in range(2):  # some state to keep
        off, n, last = sp[k]
        assert np.array_equal(ch.step(xd[off:off + n]).cpu().numpy(), outs[k])
    stats = S.upmix_stats()
    off, n, _ = sp[2]
    flush_extra = L * (ch.up.getLength() // L)

    def out(m):
        return torch.empty((m, 2), dtype=torch.int16, device="cuda")

    for o, flush in ((out(L * n + 1), False), (out(L * n - 1), False), (out(L * n + flush_extra + 1), True),
                     (out(L * n), True)):
        with pytest.raises(S.SrcdspError) as e:
            ch.step(xd[off:off + n], o, flush)
        assert e.value.code == ERR_SIZE
    # variant 2 (real int16_t) cannot feed the mixer
    c2 = make_taps("sinc", L, ntaps)
    up2 = S.FilterUpsamplingFir(c2, L, *UP_TYPES[2])
    with pytest.raises(S.SrcdspError) as e:
        S.UpsamplerMixerChain(up2, ch.mixer).step(xd[off:off + n], out(L * n))
    assert e.value.code == ERR_UNSUPPORTED
    assert S.upmix_stats() == stats
    assert ch.mixer.state()[:2] == states[1]
    xr = np.ascontiguousarray(x[:512, 0])
    assert np.array_equal(up2.step(dev(xr)).cpu().numpy(), O["strict"].up(2, L, c2).step(xr))
    # both handles go on from where they were
    for k in range(2, len(sp)):
        off, n, last = sp[k]
        assert np.array_equal(ch.step(xd[off:off + n], None, last).cpu().numpy(), outs[k]), k
        assert ch.mixer.state()[:2] == states[k], k


# ------------------------------------------------------ 5. bank
def make_bank(S, Cn, c, L=4, N=4096):
    ups, ms = [], []
    for k in range(Cn):
        ups.append(S.FilterUpsamplingFir(c, L, *UP_TYPES[0]))
        m = S.Mixer(N)
        m.reset(FREQS[k % len(FREQS)])
        ms.append(m)
    return ups, ms


def check_bank(S, O, Cn, shared, N=4096, want=2, pad=0):
    """Step a bank over the calls and compare every row, mixer state and (by a
    following single-channel call of 64 inputs) history with Cn independent
    oracle chains.  pad: extra columns per output row, which must stay untouched."""
    import torch
    L, ntaps, kind = 4, 128, "full"
    c = make_taps(kind, L, ntaps)
    ups, ms = make_bank(S, Cn, c, L, N)
    flush_extra = L * (ups[0].getLength() // L)
    xs = [signal(O, kind, 0 if shared else k) for k in range(Cn)]
    xd = dev(xs[0]) if shared else dev(np.stack(xs))
    refs = [mix_reference(O, up_reference(O, kind, L, ntaps, ch=0 if shared else k), N, FREQS[k % len(FREQS)])
            for k in range(Cn)]
    for k, (off, n, last) in enumerate(spans()):
        need = L * n + (flush_extra if last else 0)
        y = torch.full((Cn, need + pad, 2), 0x5A5A, dtype=torch.int16, device="cuda")
        xin = xd[off:off + n] if shared else xd[:, off:off + n].contiguous()
        s0 = S.upmix_stats()
        S.upmix_step_batched(ups, ms, xin, y, last)
        s1 = S.upmix_stats()
        assert tuple(b - a for a, b in zip(s0, s1)) == tuple(int(i == want) for i in range(4)), k
        yh = y.cpu().numpy()
        for ch in range(Cn):
            assert np.array_equal(yh[ch, :need], refs[ch][0][k]), (ch, k)
            assert ms[ch].state()[:2] == refs[ch][1][k], (ch, k)
        assert (yh[:, need:] == 0x5A5A).all(), k
    # histories: one more single-channel call per channel against the oracle chain run on
    extra = signal(O, kind, 7, 64)
    for ch in range(Cn):
        r = O["strict"].up(0, L, c)
        m = O["strict"].mixer(N)
        m.reset(FREQS[ch % len(FREQS)])
        x = xs[ch]
        for off, n, last in spans():
            m.step(r.step(x[off:off + n], last))
        y = S.UpsamplerMixerChain(ups[ch], ms[ch]).step(dev(extra))
        assert np.array_equal(y.cpu().numpy(), m.step(r.step(extra))), ch
        assert ms[ch].state()[:2] == m.state()[:2], ch


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("Cn", [1, 3, 8])
def test_bank_vs_independent_oracle_chains(S, O, Cn, shared):
    check_bank(S, O, Cn, shared)


def test_bank_leaves_row_padding_untouched(S, O):
    check_bank(S, O, 3, False, pad=8)


def test_bank_of_unserved_mixers_takes_the_loop(S, O):
    check_bank(S, O, 3, True, N=8192, want=3)


def test_bank_refusals(S, O):
    import torch
    from srcdsp_amd import _capi as A
    L, ntaps, n = 4, 128, 2048
    c = make_taps("full", L, ntaps)
    ups, ms = make_bank(S, 2, c)
    xd = dev(signal(O, "full"))[:n]
    y = torch.empty((2, L * n, 2), dtype=torch.int16, device="cuda")
    c_other = c.copy()
    c_other[3] += 1
    other_taps = S.FilterUpsamplingFir(c_other, L, *UP_TYPES[0])
    other_l = S.FilterUpsamplingFir(c, 2, *UP_TYPES[0])
    other_n = S.Mixer(2048)
    stats = S.upmix_stats()
    bad = [([ups[0], other_taps], ms), ([ups[0], other_l], ms), (ups, [ms[0], other_n]),
           ([ups[0], ups[0]], ms), (ups, [ms[1], ms[1]])]
    for u_, m_ in bad:
        with pytest.raises(S.SrcdspError) as e:
            S.upmix_step_batched(u_, m_, xd, y)
        assert e.value.code == A.ERR_ARG
    hu = (C.c_void_p * 2)(*[u._h.value for u in ups])
    hm = (C.c_void_p * 2)(*[m._h.value for m in ms])
    assert A.lib().srcdsp_upmix_step_batched(hu, hm, 0, xd.data_ptr(), 0, y.data_ptr(), L * n, n, 0, None) == A.ERR_ARG
    assert S.upmix_stats() == stats
    # nothing moved: the bank's first call is still the oracle's first block
    S.upmix_step_batched(ups, ms, xd, y)
    yh = y.cpu().numpy()
    x = signal(O, "full")[:n]
    for ch in range(2):
        m = O["strict"].mixer(4096)
        m.reset(FREQS[ch])
        assert np.array_equal(yh[ch], m.step(O["strict"].up(0, L, c).step(x))), ch
        assert ms[ch].state()[:2] == m.state()[:2]
