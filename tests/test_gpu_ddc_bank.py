"""The DDC bank (srcdsp_mixdecim_step_batched): C mixer -> decimator chains in
one call, on a shared input or one input per channel.  Every comparison is
bit-exact against the two oracle calls per channel (mixers.h:169-188,
dnsampling_filters.h:129-172), the mixer state included; the process-wide
counters prove which path (bank kernel / per-channel loop) served a call.

What these calls reach of the kernel: 18 to 512 tiles of 4096 samples and at
most 8 channels fill less than half of the 2048-workgroup grid, so the launcher
shrinks the channel group to 1 and every workgroup takes one tile of one
channel.  The channel loop with a group of up to 8 on one fetch, the partial
last group and a workgroup's walk over several tiles are in
test_gpu_stream_loops.py (under srcdsp_stream_set_grid_cap)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FREQS = [0.0, 0.1, -0.37, 0.5, 0.73, -0.2, 0.3, -0.45]  # frequency words: multiples of 16 and odd ones
TOTAL = 70000
# several tiles with a ragged last one, a call shorter than a lane chunk, a call
# shorter than the history (100 < 126), phase and history carried across calls
CHUNKS = [40000, 32, 100, 4100, 20000]
CI16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>")


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _chunks(total, sizes):
    out, i, k = [], 0, 0
    while i < total:
        n = min(sizes[k % len(sizes)], total - i)
        out.append((i, n))
        i += n
        k += 1
    return out


def taps(ntaps):
    from srcdsp_amd.design import hamming_sinc, q14
    # (one tap: the window's 0/0 is not a filter; unity in Q14, as test_mixdecim_chain_runtime_taps)
    return q14(hamming_sinc(ntaps)) if ntaps > 1 else np.array([16384], np.int32)


def freq(c):
    return FREQS[c % len(FREQS)]


_X, _REF = {}, {}


def signal(O, ch, n=TOTAL):
    """Full-scale input of channel `ch` (both clamps act), made once."""
    if (ch, n) not in _X:
        _X[(ch, n)] = O["strict"].gen_ci16(0xDDC, ch, 0, n, -32768, 32767)
    return _X[(ch, n)]


def reference(O, ch, ntaps, f, N=4096, M=4, variant=1, cq=None, n=TOTAL, chunks=CHUNKS, key=None):
    """The oracle's outputs and mixer states, call by call, for input channel
    `ch` through a mixer at f and the decimator; computed once and shared."""
    k = (ch, ntaps, f, N, M, variant, n, tuple(chunks), key)
    if k not in _REF:
        cq = taps(ntaps) if cq is None else cq
        om, od = O["strict"].mixer(N), O["strict"].decim(variant, M, cq)
        om.reset(f)
        x = signal(O, ch, n)
        outs, states = [], []
        for off, m in _chunks(n, chunks):
            outs.append(od.step(om.step(x[off:off + m])))
            states.append(om.state()[:2])
        _REF[k] = (outs, states)
    return _REF[k]


def make_bank(S, C, cq, N=4096, M=4, ctype="int32_t"):
    ms, ds = [], []
    for c in range(C):
        m = S.Mixer(N)
        m.reset(freq(c))
        ms.append(m)
        ds.append(S.FilterDnsamplingFir(cq, M, *CI16, ctype))
    return ms, ds


def run_bank(S, ms, ds, xd, n, chunks, M=4):
    """Step the bank over device input xd ([n, 2] shared or [C, n, 2]); the
    outputs per call as host arrays [C, m / M, 2], and the mixer states."""
    import torch
    outs, states = [], []
    for off, m in _chunks(n, chunks):
        y = torch.empty((len(ms), m // M, 2), dtype=torch.int16, device="cuda")
        xs = xd[off:off + m] if xd.dim() == 2 else xd[:, off:off + m].contiguous()
        S.mixdecim_step_batched(ms, ds, xs, y)
        outs.append(y.cpu().numpy())
        states.append([mx.state()[:2] for mx in ms])
    return outs, states


# ------------------------------------------------------ 1. shared input
@pytest.mark.parametrize("ntaps", [1, 31, 127, 128, 1024])
@pytest.mark.parametrize("C", [1, 3, 8])
def test_shared_input_bank_kernel(S, O, C, ntaps):
    cq = taps(ntaps)
    ms, ds = make_bank(S, C, cq)
    b0, l0 = S.mixdecim_batched_stats()
    outs, states = run_bank(S, ms, ds, dev(signal(O, 0)), TOTAL, CHUNKS)
    b1, l1 = S.mixdecim_batched_stats()
    assert (b1 - b0, l1 - l0) == (len(outs), 0)
    for c in range(C):
        ro, rs = reference(O, 0, ntaps, freq(c))
        for k in range(len(outs)):
            assert np.array_equal(outs[k][c], ro[k]), (c, k)
            assert states[k][c] == rs[k], (c, k)


# ------------------------------------------------- 2. independent inputs
def test_independent_inputs_bank_kernel(S, O):
    C, ntaps = 8, 127
    ms, ds = make_bank(S, C, taps(ntaps))
    x = np.stack([signal(O, c) for c in range(C)])
    b0, l0 = S.mixdecim_batched_stats()
    outs, states = run_bank(S, ms, ds, dev(x), TOTAL, CHUNKS)
    b1, l1 = S.mixdecim_batched_stats()
    assert (b1 - b0, l1 - l0) == (len(outs), 0)
    for c in range(C):
        ro, rs = reference(O, c, ntaps, freq(c))
        for k in range(len(outs)):
            assert np.array_equal(outs[k][c], ro[k]), (c, k)
            assert states[k][c] == rs[k], (c, k)


def test_independent_inputs_past_the_batch_limit(S, O):
    """65 channels: two kernel launches (64 + 1) inside one call."""
    C, ntaps, n, chunks = 65, 127, 8192 + 36, [8192, 36]
    ms, ds = make_bank(S, C, taps(ntaps))
    x = np.stack([signal(O, c, n) for c in range(C)])
    b0, l0 = S.mixdecim_batched_stats()
    outs, states = run_bank(S, ms, ds, dev(x), n, chunks)
    b1, l1 = S.mixdecim_batched_stats()
    assert (b1 - b0, l1 - l0) == (2, 0)
    for c in range(C):
        ro, rs = reference(O, c, ntaps, freq(c), n=n, chunks=chunks)
        for k in range(2):
            assert np.array_equal(outs[k][c], ro[k]), (c, k)
            assert states[k][c] == rs[k], (c, k)


# ------------------------------------------ 3. equals the single-channel API
@pytest.mark.parametrize("ntaps", [127, 1024])
def test_state_equals_single_channel_api_and_hands_over(S, O, ntaps):
    C = 3
    cq = taps(ntaps)
    x = signal(O, 0)
    xd = dev(x)
    ms, ds = make_bank(S, C, cq)
    run_bank(S, ms, ds, xd, TOTAL, CHUNKS)
    m1, d1 = make_bank(S, C, cq)
    extra = signal(O, 1, 4096)
    for c in range(C):
        chain = S.MixerDecimatorChain(m1[c], d1[c])
        om, od = O["strict"].mixer(4096), O["strict"].decim(1, 4, cq)
        om.reset(freq(c))
        for off, m in _chunks(TOTAL, CHUNKS):
            chain.step(xd[off:off + m])
            od.step(om.step(x[off:off + m]))
        assert ms[c].state()[:2] == m1[c].state()[:2] == om.state()[:2], c
        sb, s1 = ds[c].state(), d1[c].state()
        assert sb["coeff_scaling"] == s1["coeff_scaling"] and sb["left_shift"] == s1["left_shift"]
        assert np.array_equal(sb["history"], s1["history"]), c
        # one further single-channel step on the batched handles
        y = S.MixerDecimatorChain(ms[c], ds[c]).step(dev(extra))
        assert np.array_equal(y.cpu().numpy(), od.step(om.step(extra))), c
        assert ms[c].state()[:2] == om.state()[:2], c


# ------------------------------------------------- 4. fallback shapes
@pytest.mark.parametrize("case", ["N1000", "M2", "M8", "variant2", "wide_taps", "in_offset"])
def test_fallback_shapes_take_the_loop_and_stay_exact(S, O, case):
    C, ntaps, n, chunks = 3, 63, 20000, [12000, 8, 7992]
    N = 1000 if case == "N1000" else 4096
    M = {"M2": 2, "M8": 8}.get(case, 4)
    variant, ctype = (2, "int16_t") if case == "variant2" else (1, "int32_t")
    cq = taps(ntaps)
    if case == "wide_taps":  # |c| >= 2^15: not the dot2 tap pairs
        cq = cq.copy()
        cq[0] = 1 << 15
    if variant == 2:
        cq = cq.astype(np.int16)
    ms, ds = make_bank(S, C, cq, N=N, M=M, ctype=ctype)
    x = signal(O, 0, n + 4)
    ioff = 1 if case == "in_offset" else 0  # a view 4 bytes off 16-byte alignment
    xd = dev(x)[ioff:ioff + n]
    b0, l0 = S.mixdecim_batched_stats()
    outs, states = run_bank(S, ms, ds, xd, n, chunks, M=M)
    b1, l1 = S.mixdecim_batched_stats()
    assert (b1 - b0, l1 - l0) == (0, len(outs))
    for c in range(C):
        om, od = O["strict"].mixer(N), O["strict"].decim(variant, M, cq)
        om.reset(freq(c))
        for k, (off, m) in enumerate(_chunks(n, chunks)):
            assert np.array_equal(outs[k][c], od.step(om.step(x[ioff + off:ioff + off + m]))), (c, k)
            assert states[k][c] == om.state()[:2], (c, k)


def test_work_bound_between_bank_and_loop(S, O):
    """n_in x taps = 2^31 is the last call the bank kernel takes (longer ones
    measured faster through the loop): 1024 taps at 2^21 samples (bank) and at
    2^21 + 4 (loop), both exact.  One oracle run serves both: the shorter
    call's outputs are a prefix of the longer one's."""
    import torch
    C, ntaps, n = 2, 1024, 1 << 21
    cq = taps(ntaps)
    x = signal(O, 3, n + 4)
    xd = dev(x)
    refs = []
    for c in range(C):
        om, od = O["strict"].mixer(4096), O["strict"].decim(1, 4, cq)
        om.reset(freq(c + 1))
        refs.append(od.step(om.step(x)))
    for m, want in ((n, (1, 0)), (n + 4, (0, 1))):
        ms, ds = [], []
        for c in range(C):
            mx = S.Mixer(4096)
            mx.reset(freq(c + 1))
            ms.append(mx)
            ds.append(S.FilterDnsamplingFir(cq, 4, *CI16, "int32_t"))
        y = torch.empty((C, m // 4, 2), dtype=torch.int16, device="cuda")
        b0, l0 = S.mixdecim_batched_stats()
        S.mixdecim_step_batched(ms, ds, xd[:m], y)
        b1, l1 = S.mixdecim_batched_stats()
        assert (b1 - b0, l1 - l0) == want, m
        for c in range(C):
            assert np.array_equal(y[c].cpu().numpy(), refs[c][:m // 4]), (m, c)
            assert ms[c].state()[0] == (m % 4096) * ms[c].state()[1] % 4096, (m, c)


# ------------------------------------------------- 5. argument errors
def test_argument_errors_change_no_state(S, O):
    import torch
    from srcdsp_amd._capi import ERR_ARG
    cq = taps(31)
    ms, ds = make_bank(S, 2, cq)
    x = signal(O, 0, 4096)
    xd = dev(x)
    y = torch.empty((2, 1024, 2), dtype=torch.int16, device="cuda")
    S.mixdecim_step_batched(ms, ds, xd, y)  # some state to keep
    torch.cuda.synchronize()

    def snapshot():
        return [m.state()[:2] for m in ms], [d.state()["history"].copy() for d in ds]

    before = snapshot()
    other_taps = S.FilterDnsamplingFir(taps(33), 4, *CI16, "int32_t")
    other_n = S.Mixer(2048)
    other_n.reset(0.1)
    bad = [
        (ms, [ds[0], other_taps], xd, y),   # decimators with different taps
        ([ms[0], other_n], ds, xd, y),      # mixers with different N
        ([ms[0], ms[0]], ds, xd, y),        # a mixer listed twice
        (ms, [ds[1], ds[1]], xd, y),        # a decimator listed twice
    ]
    stats = S.mixdecim_batched_stats()
    for m_, d_, x_, y_ in bad:
        with pytest.raises(S.SrcdspError) as e:
            S.mixdecim_step_batched(m_, d_, x_, y_)
        assert e.value.code == ERR_ARG
    # n_in % M != 0: straight through the C ABI (the Python wrapper refuses the shape earlier)
    import ctypes as C
    from srcdsp_amd import _capi as A
    hm = (C.c_void_p * 2)(*[m._h.value for m in ms])
    hd = (C.c_void_p * 2)(*[d._h.value for d in ds])
    rc = A.lib().srcdsp_mixdecim_step_batched(hm, hd, 2, xd.data_ptr(), 0, y.data_ptr(), 1024, 4094, None)
    assert rc == ERR_ARG
    with pytest.raises(ValueError):
        S.mixdecim_step_batched(ms, ds, xd[:4094], y)
    with pytest.raises(ValueError):
        S.mixdecim_step_batched(ms, ds[:1], xd, y)
    assert S.mixdecim_batched_stats() == stats
    after = snapshot()
    assert before[0] == after[0]
    assert all(np.array_equal(p, q) for p, q in zip(before[1], after[1]))
    assert other_n.state()[:2] == (0, other_n.state()[1])
    assert not other_taps.state()["history"].any()


# ------------------------------------------------------ 6. two streams
def test_batched_then_single_channel_on_another_stream(S, O):
    """A batched call on a side stream, then a single-channel call on the
    default stream on one of its handles, with no host synchronise between."""
    import torch
    C, ntaps, n = 3, 127, 1 << 18
    cq = taps(ntaps)
    x = signal(O, 2, 2 * n)
    xd = dev(x)
    ms, ds = make_bank(S, C, cq)
    side = torch.cuda.Stream()
    yb = torch.empty((C, n // 4, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        S.mixdecim_step_batched(ms, ds, xd[:n], yb)
    y1 = S.MixerDecimatorChain(ms[1], ds[1]).step(xd[n:])  # default stream
    torch.cuda.synchronize()
    for c in range(C):
        om, od = O["strict"].mixer(4096), O["strict"].decim(1, 4, cq)
        om.reset(freq(c))
        assert np.array_equal(yb[c].cpu().numpy(), od.step(om.step(x[:n]))), c
        if c == 1:
            assert np.array_equal(y1.cpu().numpy(), od.step(om.step(x[n:])))
        assert ms[c].state()[:2] == om.state()[:2], c
