"""The interpolator -> decimator chain (srcdsp_resample_step,
srcdsp_resample_step_batched): the rational L/M rate change.  Every comparison
is bit-exact against the oracle's two calls (upsampling_filters.h:149-233 then
dnsampling_filters.h:129-172); after every call the decimator's state
(coeffScaling, leftShift, history) and the interpolator's next-call behaviour
equal those of a twin pair of handles stepped through srcdsp_up_step and
srcdsp_decim_step; the process-wide counters prove which path served a call.

The module forces the fused kernel onto every shape it takes
(resample_set_min_tiles(1)), so the paths tested are decided by shape alone,
not by the measured routing.

A tile is 2048 inputs.  A stream of about 9000 inputs is cut into calls of two
tiles and a ragged third, one lane's worth, fewer inputs than the
interpolator's history, L n < N_d - 1 (the sliding rule of DESIGN 9), one tile
(exactly 2048 where 2048 L is a multiple of M) and a flushing rest.  Every
call has L n a multiple of M and every offset is a multiple of 4 samples."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_upmix import UP_TYPES, dev, make_taps, signal

pytestmark = pytest.mark.gpu

DEC_TYPES = {0: ("complex<float>", "complex<float>", "complex<float>", "float"),
             1: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t"),
             2: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int16_t"),
             3: ("complex<int32_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")}
FUSED, PAIR, BANK, LOOP = range(4)


def force_fused(S):
    S.resample_set_min_tiles(1)
    yield
    S.resample_set_min_tiles(0)


@pytest.fixture(scope="module", autouse=True)
def fused_on_every_shape_it_takes(S):
    yield from force_fused(S)


def decim_taps(kind, M, ntaps):
    """"sinc": a Q14 decimation low-pass; "full": random full-range int16 taps
    (the seed apart from the interpolator's)."""
    if kind == "sinc":
        from srcdsp_amd.design import hamming_sinc, q14
        return q14(hamming_sinc(ntaps, 0.48 / max(M, 2)))
    c = np.random.default_rng(77000 + 1000 * M + ntaps).integers(-32768, 32768, size=ntaps).astype(np.int32)
    c[0], c[-1] = 32767, -32768
    return c


def shape_calls(L, Nu, M, flush_len=None):
    """The call lengths of a shape: [(offset, n, flush)], about 9000 inputs."""
    H = (Nu if flush_len is None else flush_len) // L
    g = M // math.gcd(L, M)           # L n % M == 0  <=>  n % g == 0
    q = g * 4 // math.gcd(g, 4)       # and offsets stay multiples of 4 samples

    def r(n):
        return max(q, n // q * q)

    calls = [r(4100 + q), r(8), r(20), q, 2048 if 2048 % q == 0 else r(2048)]
    rest = 9000 - sum(calls)
    rest += (-(rest + H)) % g         # the flushed call: L (n + length / L) % M == 0
    calls.append(rest)
    off, out = 0, []
    for i, n in enumerate(calls):
        assert (L * (n + (H if i == len(calls) - 1 else 0))) % M == 0 and off % 4 == 0
        out.append((off, n, i == len(calls) - 1))
        off += n
    return out, off


def oracle_chain(O, x, calls, uvar, L, cu, dvar, M, cd, ls):
    up, dec = O["strict"].up(uvar, L, cu), O["strict"].decim(dvar, M, cd)
    dec.set_left_shift(ls)
    return [dec.step(up.step(x[off:off + n], last)) for off, n, last in calls]


def clamp_share(outs):
    y = np.concatenate(outs)
    return float(np.mean(np.abs(y.astype(np.int32)) == 32767))


_REF = {}


def reference(O, kind, L, Nu, M, Nd, uvar=0, dvar=1, cu=None, cd=None, tag=None, ls=None):
    """x, calls, taps, the decimator's left shift and the oracle's output of
    every call; computed once per case.  "full": the left shift is the smallest
    for which at least 10 % of the oracle's outputs sit on +-32767 (the
    interpolator's clamp bites at any shift, the decimator's only then), and
    that share is below 95 % -- asserted on the oracle alone.  A caller that
    passes its own taps (cu, cd) may pass the left shift too (ls): it is then
    used as given; any kind but "full" takes the moderate input of "sinc"."""
    key = (kind, L, Nu, M, Nd, uvar, dvar, tag)
    if key not in _REF:
        cu = make_taps(kind, L, Nu) if cu is None else cu
        cd = decim_taps(kind, M, Nd) if cd is None else cd
        calls, total = shape_calls(L, Nu, M)
        x = signal(O, "full" if kind == "full" else "sinc", 0, total + 8)
        given = ls is not None
        ls = ls if given else 0
        outs = oracle_chain(O, x, calls, uvar, L, cu, dvar, M, cd, ls)
        if kind == "full" and not given:
            while clamp_share(outs) < 0.10:
                ls += 1
                assert ls < 32, "no left shift puts 10 % of the outputs on the clamp"
                outs = oracle_chain(O, x, calls, uvar, L, cu, dvar, M, cd, ls)
            share = clamp_share(outs)
            print(f"shape {(L, Nu, M, Nd)}: left shift {ls}, share on +-32767 {share:.3f}")
            assert 0.10 <= share <= 0.95, (ls, share)
        _REF[key] = dict(x=x, calls=calls, cu=cu, cd=cd, ls=ls, outs=outs)
    return _REF[key]


def handles(S, ref, L, M, uvar=0, dvar=1):
    cu = ref["cu"].astype(np.int16) if uvar == 1 else ref["cu"]
    cd = ref["cd"].astype(np.int16) if dvar == 2 else ref["cd"]
    up = S.FilterUpsamplingFir(cu, L, *UP_TYPES[uvar])
    dec = S.FilterDnsamplingFir(cd, M, *DEC_TYPES[dvar])
    dec.set_left_shift(ref["ls"])
    return up, dec


def same_state(S, up, dec, tup, tdec, ls, probe, where):
    a, b = dec.state(), tdec.state()
    assert a["coeff_scaling"] == b["coeff_scaling"] and a["left_shift"] == b["left_shift"] == ls, where
    assert np.array_equal(a["history"], b["history"]), where
    # the interpolator's next call, on copies
    ya, yb = copy.copy(up).step(probe), copy.copy(tup).step(probe)
    assert np.array_equal(ya.cpu().numpy(), yb.cpu().numpy()), where


GUARD_VALUE = 0x5A5A


def run_and_check(S, ref, L, M, want, uvar=0, dvar=1, ioff=0, ooff=0, guard=0):
    """Step the chain over the calls; after each: outputs, which counter rose
    (want: index into resample_stats()), both handles' state against twin
    handles stepped through the two single operators, and the samples around
    the output (guard more behind it) keep their fill value."""
    import torch
    up, dec = handles(S, ref, L, M, uvar, dvar)
    tup, tdec = handles(S, ref, L, M, uvar, dvar)
    rs = S.RationalResampler(up, dec)
    xd = dev(ref["x"])
    probe = xd[:64]
    for k, (off, n, last) in enumerate(ref["calls"]):
        xs = xd[ioff + off:ioff + off + n]
        want_y = ref["outs"][k]
        buf = torch.full((len(want_y) + 4 + guard, 2), GUARD_VALUE, dtype=torch.int16, device="cuda")
        y = buf[ooff:ooff + len(want_y)]
        s0 = S.resample_stats()
        rs.step(xs, y, last)
        s1 = S.resample_stats()
        assert np.array_equal(y.cpu().numpy(), want_y), k
        assert (buf[:ooff] == GUARD_VALUE).all() and (buf[ooff + len(want_y):] == GUARD_VALUE).all(), k
        assert tuple(b - a for a, b in zip(s0, s1)) == tuple(int(i == want) for i in range(4)), k
        yt = tdec.step(tup.step(xs, None, last))
        assert np.array_equal(yt.cpu().numpy(), want_y), k
        same_state(S, up, dec, tup, tdec, ref["ls"], probe, k)


# ------------------------------------------------------ 1. fused path
# (L, N_u, M, N_d); (4,128) (2,64) (8,128): pairs per phase compiled in, the others at run time
SHAPES = [(4, 128, 3, 96), (4, 128, 4, 127), (2, 64, 3, 63), (3, 96, 2, 64), (8, 128, 5, 100), (5, 40, 8, 128),
          (4, 128, 1, 31), (7, 56, 6, 255)]


@pytest.mark.parametrize("kind", ["sinc", "full"])
@pytest.mark.parametrize("L,Nu,M,Nd", SHAPES)
def test_fused_kernel_vs_oracle(S, O, L, Nu, M, Nd, kind):
    run_and_check(S, reference(O, kind, L, Nu, M, Nd), L, M, FUSED)


def test_call_plan_has_the_cases_it_names():
    """The cut of the stream: more than two tiles, one lane, fewer inputs than
    the interpolator's history and L n < N_d - 1 where the shape allows them,
    exactly one tile where 2048 L is a multiple of M."""
    sliding = short = 0
    for L, Nu, M, Nd in SHAPES:
        calls, total = shape_calls(L, Nu, M)
        ns = [n for _, n, _ in calls]
        assert ns[0] > 4096 and ns[0] % 2048 and 8900 <= total <= 9100, (L, M, ns)
        assert all((L * n) % M == 0 for n in ns[:-1])
        if (2048 * L) % M == 0 and M in (1, 2, 4, 8):
            assert 2048 in ns
        sliding += any(L * n < Nd - 1 for n in ns)
        if min(ns) < Nu // L - 1:
            short += 1
    assert sliding >= 6 and short >= 5, (sliding, short)


# ------------------------------------------------------ 2. continuity
@pytest.mark.parametrize("fused_first", [True, False])
def test_state_hands_over_between_chain_and_single_operators(S, O, fused_first):
    L, Nu, M, Nd = 4, 128, 3, 96
    ref = reference(O, "full", L, Nu, M, Nd)
    up, dec = handles(S, ref, L, M)
    rs = S.RationalResampler(up, dec)
    xd = dev(ref["x"])
    order = [fused_first, fused_first, not fused_first, fused_first, not fused_first, fused_first]
    for k, (off, n, last) in enumerate(ref["calls"]):
        xs = xd[off:off + n]
        y = rs.step(xs, None, last) if order[k] else dec.step(up.step(xs, None, last))
        assert np.array_equal(y.cpu().numpy(), ref["outs"][k]), k


# ------------------------------------------------------ 3. pair path
PAIR_CASES = ["up_variant1", "decim_variant2", "wide_tap_up", "wide_tap_decim", "L9", "M16", "Nd_above_cap",
              "in_offset", "out_offset"]


@pytest.mark.parametrize("case", PAIR_CASES)
def test_other_shapes_take_the_pair_and_stay_exact(S, O, case):
    L, Nu, M, Nd = 4, 128, 3, 96
    uvar, dvar, cu, cd = 0, 1, None, None
    if case == "up_variant1":
        uvar = 1
    elif case == "decim_variant2":
        dvar = 2
    elif case == "wide_tap_up":      # beyond int16: not the dot2 tap pairs
        cu = make_taps("full", L, Nu).copy()
        cu[5] = 1 << 20
    elif case == "wide_tap_decim":
        cd = decim_taps("full", M, Nd).copy()
        cd[5] = 1 << 20
    elif case == "L9":
        L, Nu = 9, 144
    elif case == "M16":
        M = 16
    elif case == "Nd_above_cap":
        Nd = S.resample_geometry()[1] + 1
    ref = reference(O, "full", L, Nu, M, Nd, uvar, dvar, cu, cd, tag=case)
    # a view one sample (4 bytes) off 16-byte alignment
    if case == "in_offset":
        calls = ref["calls"]
        x = ref["x"]
        ref = dict(ref, outs=oracle_chain(O, x[1:], calls, uvar, L, ref["cu"], dvar, M, ref["cd"], ref["ls"]))
    run_and_check(S, ref, L, M, PAIR, uvar, dvar, ioff=int(case == "in_offset"), ooff=int(case == "out_offset"))


def test_measured_routing_sends_only_the_winning_classes_to_the_kernel(S, O):
    """Without the test hook: L/M = 4/3 goes to the fused kernel from 2048
    tiles on and to the pair below; L/M = 4/4, where the kernel measured
    slower, to the pair at any length.  Outputs equal the two single calls."""
    import torch
    n = 2049 * 2048 - 2040  # 2049 tiles, 4 n a multiple of 3 and of 4
    assert (4 * n) % 12 == 0 and -(-n // 2048) == 2049
    x = torch.randint(-32768, 32768, (n, 2), dtype=torch.int16, device="cuda")
    S.resample_set_min_tiles(0)
    try:
        for (L, Nu, M, Nd), m, want in (((4, 128, 3, 96), n, FUSED), ((4, 128, 3, 96), 4104, PAIR),
                                        ((4, 128, 4, 127), n, PAIR)):
            ref = reference(O, "full", L, Nu, M, Nd)
            up, dec = handles(S, ref, L, M)
            tup, tdec = handles(S, ref, L, M)
            s0 = S.resample_stats()
            y = S.RationalResampler(up, dec).step(x[:m])
            s1 = S.resample_stats()
            assert tuple(b - a for a, b in zip(s0, s1)) == tuple(int(i == want) for i in range(4)), (L, M, m)
            assert torch.equal(y, tdec.step(tup.step(x[:m]))), (L, M, m)
            same_state(S, up, dec, tup, tdec, ref["ls"], x[:64], (L, M, m))
    finally:
        S.resample_set_min_tiles(1)


# ------------------------------------------------------ 4. refusals
def test_refusals_change_no_state(S, O):
    import torch
    from srcdsp_amd import _capi as A
    L, Nu, M, Nd = 4, 128, 3, 96
    ref = reference(O, "full", L, Nu, M, Nd)
    up, dec = handles(S, ref, L, M)
    rs = S.RationalResampler(up, dec)
    xd = dev(ref["x"])
    calls = ref["calls"]
    for k in range(2):  # some state to keep
        off, n, last = calls[k]
        assert np.array_equal(rs.step(xd[off:off + n]).cpu().numpy(), ref["outs"][k])
    stats, state = S.resample_stats(), dec.state()
    off, n, _ = calls[2]

    def out(m):
        return torch.empty((m, 2), dtype=torch.int16, device="cuda")

    def refused(r, x, o, flush, code):
        with pytest.raises(S.SrcdspError) as e:
            r.step(x, o, flush)
        assert e.value.code == code

    assert (L * 8) % M
    refused(rs, xd[off:off + 8], out(L * 8 // M), False, A.ERR_SIZE)         # L n % M != 0
    refused(rs, xd[off:off + n], out(L * n // M + 1), False, A.ERR_SIZE)     # a wrong n_out
    refused(rs, xd[off:off + n], out(L * n // M - 1), False, A.ERR_SIZE)
    refused(rs, xd[off:off + n], out(L * n // M), True, A.ERR_SIZE)          # flushing needs length / L more
    up2 = S.FilterUpsamplingFir(make_taps("sinc", L, Nu), L, *UP_TYPES[2])   # real int16_t
    refused(S.RationalResampler(up2, dec), xd[off:off + n], out(L * n // M), False, A.ERR_UNSUPPORTED)
    for dvar in (0, 3):
        taps = np.ones(Nd, np.float32) if dvar == 0 else decim_taps("full", M, Nd)
        d2 = S.FilterDnsamplingFir(taps, M, *DEC_TYPES[dvar])
        refused(S.RationalResampler(up, d2), xd[off:off + n], out(L * n // M), False, A.ERR_UNSUPPORTED)
    o = out(L * n // M)
    lib = A.lib()
    for hu, hd in ((None, dec._h), (up._h, None), (None, None)):
        assert lib.srcdsp_resample_step(hu, hd, xd.data_ptr(), n, o.data_ptr(), L * n // M, 0, None) == A.ERR_ARG
    assert S.resample_stats() == stats
    after = dec.state()
    assert after["coeff_scaling"] == state["coeff_scaling"] and after["left_shift"] == state["left_shift"]
    assert np.array_equal(after["history"], state["history"])
    # n_in = 0 without flush: fine, and nothing moves
    rs.step(xd[:0], out(0))
    assert np.array_equal(dec.state()["history"], state["history"])
    # both handles go on from where they were
    for k in range(2, len(calls)):
        off, n, last = calls[k]
        assert np.array_equal(rs.step(xd[off:off + n], None, last).cpu().numpy(), ref["outs"][k]), k


# ------------------------------------------------------ 5. bank
BANK_N = 4104  # two tiles and a ragged third with 4 n a multiple of 3 (4100 is not)


def make_bank(S, ref, Cn, L, M):
    pairs = [handles(S, ref, L, M) for _ in range(Cn)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def bank_rows(O, Cn, n0, n1):
    xs = np.stack([signal(O, "full", k, n0 + n1) for k in range(Cn)])
    return xs


def check_bank(S, O, Cn, want, in_pad=0):
    """A first call gives every channel its own histories; the second, of
    BANK_N inputs, is compared with the loop of single calls on twin handles:
    rows, both handles' state, and one count on the wanted path."""
    import torch
    L, Nu, M, Nd = 4, 128, 3, 96
    ref = reference(O, "full", L, Nu, M, Nd)
    n0 = 24
    ups, decs = make_bank(S, ref, Cn, L, M)
    tups, tdecs = make_bank(S, ref, Cn, L, M)
    xs = bank_rows(O, Cn, n0, BANK_N)
    xd = dev(xs)
    wide = torch.zeros((Cn, BANK_N + in_pad, 2), dtype=torch.int16, device="cuda")
    wide[:, :BANK_N] = xd[:, n0:]
    x1 = wide[:, :BANK_N]
    assert (x1.stride(0) * 2) % 16 == (0 if in_pad == 0 else 8)
    for c in range(Cn):  # distinct histories, by single calls
        for u, d in ((ups[c], decs[c]), (tups[c], tdecs[c])):
            S.RationalResampler(u, d).step(xd[c, :n0].contiguous())
    n_out = L * BANK_N // M
    y = torch.full((Cn, n_out + 4, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    s0 = S.resample_stats()
    S.resample_step_batched(ups, decs, x1, y)
    s1 = S.resample_stats()
    d = tuple(b - a for a, b in zip(s0, s1))
    assert d[BANK] + d[LOOP] == 1 and d[want] == 1 and d[FUSED] == d[PAIR] == 0, d
    yh = y.cpu().numpy()
    assert (yh[:, n_out:] == 0x5A5A).all()
    probe = xd[0, :64].contiguous()
    for c in range(Cn):
        yt = S.RationalResampler(tups[c], tdecs[c]).step(xd[c, n0:].contiguous())
        assert np.array_equal(yh[c, :n_out], yt.cpu().numpy()), c
        same_state(S, ups[c], decs[c], tups[c], tdecs[c], ref["ls"], probe, c)
    for c in range(min(Cn, 3)):  # and the oracle, on a few rows
        calls = [(0, n0, False), (n0, BANK_N, False)]
        want_y = oracle_chain(O, xs[c], calls, 0, L, ref["cu"], 1, M, ref["cd"], ref["ls"])[1]
        assert np.array_equal(yh[c, :n_out], want_y), c


@pytest.mark.parametrize("Cn", [3, 65])
def test_bank_vs_loop_of_single_calls(S, O, Cn):
    check_bank(S, O, Cn, BANK)


def test_bank_with_a_row_stride_off_16_bytes_takes_the_loop(S, O):
    check_bank(S, O, 3, LOOP, in_pad=2)


def test_bank_refuses_a_handle_listed_twice(S, O):
    import torch
    from srcdsp_amd import _capi as A
    L, Nu, M, Nd = 4, 128, 3, 96
    ref = reference(O, "full", L, Nu, M, Nd)
    ups, decs = make_bank(S, ref, 2, L, M)
    xd = dev(bank_rows(O, 2, 0, 24))
    y = torch.empty((2, L * 24 // M, 2), dtype=torch.int16, device="cuda")
    stats = S.resample_stats()
    other_m = S.FilterDnsamplingFir(ref["cd"], 4, *DEC_TYPES[1])
    other_l = S.FilterUpsamplingFir(make_taps("full", 2, 64), 2, *UP_TYPES[0])
    for u_, d_ in (([ups[0], ups[0]], decs), (ups, [decs[1], decs[1]]), (ups, [decs[0], other_m]),
                   ([ups[0], other_l], decs)):
        with pytest.raises(S.SrcdspError) as e:
            S.resample_step_batched(u_, d_, xd, y)
        assert e.value.code == A.ERR_ARG
    assert S.resample_stats() == stats
    S.resample_step_batched(ups, decs, xd, y)  # nothing moved: the first call is the oracle's first block
    for c in range(2):
        want_y = oracle_chain(O, signal(O, "full", c, 24), [(0, 24, False)], 0, L, ref["cu"], 1, M, ref["cd"], ref["ls"])
        assert np.array_equal(y[c].cpu().numpy(), want_y[0]), c
