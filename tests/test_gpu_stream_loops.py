"""The persistent receive kernels' tile loops, and the DDC bank's channel groups.

Every streaming kernel of the receive side runs on min(tiles, a product grid of
1024..2048) workgroups, so in calls of under a few million samples every
workgroup owns exactly one tile and the code that carries a workgroup from one
tile to the next -- the prefetch of the next tile behind the current one's
taps, the per/rem split of the tile range, the fused mixer's per-tile phase
advance, the bank's one fetch serving a group of channels -- never runs.  Here
the grid is capped (srcdsp_stream_set_grid_cap) at 16 (a multiple of 8, as the
product grids: xcd_tile's r = 0) and, for one case per kernel family, at 11
(r = 3: both arms of x < r), and every instantiation is stepped through

    37 tiles + 3 M samples   (38 tiles, the last one ragged; 38 = 2*16 + 6 =
                              3*11 + 5: both b < rem arms, two to four tiles
                              per workgroup, tile 0's owner among them),
    one lane chunk,
    a call shorter than the history,
    exactly 9 tiles          (under both caps: no workgroup loops),
    20 tiles,

every output bit for bit the oracle's, written into a poisoned buffer (a tile
nobody wrote cannot pass on stale memory) with 64 samples of guard band behind
it, the decimator history after every call, the mixer state where a mixer is
fused, and the process-wide counters (srcdsp_stream_grid_stats) proving around
every call that it was one persistent launch, looping exactly when it has more
tiles than the cap allows workgroups.

Not reachable: none of the instantiations is; decim_stream_cf32's Q0 = false
forms are reached through the public calls -- a constructor whose taps sum to 2
or more (coeffScaling >= 1) or setLeftShiftBy2 make (shift & 31) != 0.
"""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_ddc_bank import CHUNKS, FREQS
from test_gpu_ddc_bank import taps as bank_taps

pytestmark = pytest.mark.gpu

GUARD = 64
POISON_F = np.float32(-1.5e30)   # no quantised output has this value
POISON_I = 0x5A5A
CI16 = ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t")
CAPS = (16, 11)


@pytest.fixture
def cap(S):
    """Set the grid cap for one test; the product grids are back afterwards."""
    def set_cap(n):
        S.stream_set_grid_cap(n)
        assert S.stream_get_grid_cap() == n
        return n
    yield set_cap
    S.stream_set_grid_cap(0)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------- call pattern
def short_call(ntaps, M):
    """The longest call of whole outputs shorter than the history (ntaps - 1
    samples); with no such call (ntaps - 1 <= M), one output."""
    return max(M, (ntaps - 2) // M * M)


def call_pattern(T, M, lane_chunk, ntaps):
    calls = [37 * T + 3 * M, lane_chunk, short_call(ntaps, M), 9 * T, 20 * T]
    assert all(n > 0 and n % M == 0 for n in calls) and T % M == 0
    assert ntaps - 1 <= M or calls[2] < ntaps - 1
    return calls


def tiles(n, T):
    return -(-n // T)


def test_pattern_gives_every_workgroup_two_or_three_tiles():
    """The arithmetic the module relies on, for both caps (no GPU work)."""
    for T, M in ((8192, 4), (4096, 1), (6144, 12), (2048, 1)):
        assert [tiles(n, T) for n in call_pattern(T, M, M, 127)] == [38, 1, 1, 9, 20]
    for nb in CAPS:
        per, rem = divmod(38, nb)
        assert per >= 2 and 0 < rem < nb          # both arms of b < rem, tile 0's owner goes on to tile 1
        assert 9 < nb < 20
    assert (16 >> 3, 16 & 7) == (2, 0) and (11 >> 3, 11 & 7) == (1, 3)  # xcd_tile's q, r


# ------------------------------------------------------ poisoned output, guard
def poisoned(kind, n, rows=1, stride=None):
    """A device buffer of `rows` rows of `stride` >= n + GUARD samples, every
    byte poison."""
    import torch
    stride = n + GUARD if stride is None else stride
    assert stride >= n + GUARD
    if kind == "cf32":
        buf = torch.empty((rows, stride), dtype=torch.complex64, device="cuda")
        torch.view_as_real(buf).fill_(float(POISON_F))
    else:
        buf = torch.full((rows, stride, 2), POISON_I, dtype=torch.int16, device="cuda")
    return buf


def check_rows(buf, kind, n, wants, what):
    """Row r of buf holds wants[r] bit for bit in its first n samples and
    untouched poison behind them."""
    h = buf.cpu().numpy()
    for r, want in enumerate(wants):
        assert len(want) == n, what
        if kind == "cf32":
            got, guard = h[r, :n], h[r, n:].view(np.float32)
            same = np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
            clean = bool((guard == POISON_F).all())
        else:
            got, guard = h[r, :n], h[r, n:]
            same = np.array_equal(got, want)
            clean = bool((guard == POISON_I).all())
        if not same:
            g2 = got.view(np.uint32).reshape(n, -1) if kind == "cf32" else got
            w2 = np.ascontiguousarray(want).view(np.uint32).reshape(n, -1) if kind == "cf32" else want
            bad = np.flatnonzero((g2 != w2).any(axis=1))
            raise AssertionError(f"{what} row {r}: {len(bad)} of {n} outputs differ, first at {bad[0]}, last at {bad[-1]}")
        assert clean, f"{what} row {r}: the guard band behind the output was written"


class History:
    """The decimator's history as the reference keeps it: the last H samples
    of everything the filter has been fed, zeros before that."""

    def __init__(self, H, like):
        self.H = H
        self.buf = np.zeros((H,) + like.shape[1:], like.dtype)

    def push(self, x):
        if self.H:
            self.buf = np.concatenate([self.buf, x])[-self.H:]

    def check(self, filt, what):
        if self.H:
            assert filt.state()["history"].tobytes() == np.ascontiguousarray(self.buf).tobytes(), what


def drive(S, cap_n, T, calls, x, kind, step, ref_step, after=None):
    """Step the calls over x: step(device input, device output view) on the
    GPU, ref_step(host input) the oracle's output; counters around each call."""
    off = 0
    for k, n in enumerate(calls):
        xs = x[off:off + n]
        off += n
        want = ref_step(xs)
        buf = poisoned(kind, len(want))
        xd = dev(xs)
        a0, l0 = S.stream_grid_stats()
        step(xd, buf[0, :len(want)])
        a1, l1 = S.stream_grid_stats()
        what = f"call {k} of {n} samples ({tiles(n, T)} tiles, cap {cap_n})"
        assert (a1 - a0, l1 - l0) == (1, int(tiles(n, T) > cap_n)), what
        check_rows(buf, kind, len(want), [want], what)
        if after:
            after(k, xs, what)
    assert off <= len(x)


def with_caps(all_cases, at_11):
    """Every case at cap 16, the chosen ones at cap 11 too."""
    assert all(c in all_cases for c in at_11)
    return [(16, c) for c in all_cases] + [(11, c) for c in at_11]


def ids(params):
    return ["cap%d-%s" % (c, "-".join(str(v) for v in case)) for c, case in params]


# ================================================================ decim_stream_cf32
CF32_COMPILED = [(127, 4), (128, 4), (63, 4), (64, 4), (127, 8), (128, 8), (255, 8), (256, 8),
                 (127, 16), (128, 16), (255, 16), (256, 16), (63, 2), (64, 2), (127, 2), (128, 2),
                 (63, 3), (64, 3), (127, 3), (128, 3), (63, 1), (64, 1)]   # launch_cf32_compiled
CF32_RT_M = [1, 2, 3, 4, 6, 8, 12, 16]                                    # launch_cf32_rt
# runtime taps: a short filter (M = 6 takes this kernel from 48 taps on) and one
# at or next to 1024, the halo the register prefetch is sized for
CF32_RT = [(49 if M == 6 else 13, M) for M in CF32_RT_M] + [(1021 if M in (1, 3, 6, 12) else 1024, M) for M in CF32_RT_M]
CF32_CASES = [(n, M, fp) for n, M in CF32_COMPILED + CF32_RT for fp in ("fma", "strict")]
CF32_PARAMS = with_caps(CF32_CASES, [(127, 4, "fma"), (1021, 3, "strict")])


def cf32_geometry(M):
    R = 8 if M == 1 else (4 if M <= 3 else 16 // M)   # cf32_r<M>()
    return M * 512 * R, M * R                         # input samples per tile, per lane chunk


def cf32_filter(S, O, c, M, fp, abs_binding="int"):
    if M == 1:
        return (S.FilterFir(c, fp=fp, abs_binding=abs_binding),
                O[fp].fir(0, c, abs_mode=int(abs_binding == "fabs")))
    return (S.FilterDnsamplingFir(c, M, fp=fp, abs_binding=abs_binding),
            O[fp].decim(0, M, c, abs_mode=int(abs_binding == "fabs")))


def cf32_taps(ntaps, M):
    from srcdsp_amd.design import hamming_sinc
    if (ntaps, M) in CF32_COMPILED:   # the design filter; an even count is the odd one with a trailing zero tap
        c = hamming_sinc(ntaps - (ntaps % 2 == 0))
        return np.concatenate([c, [0.0]]).astype(np.float32) if ntaps % 2 == 0 else c
    rng = np.random.default_rng(M * 7919 + ntaps)
    return (rng.standard_normal(ntaps) / max(2, ntaps) ** 0.5).astype(np.float32)


@pytest.mark.parametrize("cap_n,case", CF32_PARAMS, ids=ids(CF32_PARAMS))
def test_cf32_tile_loop(S, O, cap, cap_n, case):
    """decim_stream_cf32 at every compiled (NT, M), and with the tap count at
    run time at every M, in both float contracts: the grid-stride loop body
    (stage_load(tile + nb) ahead of do_tile<WHOLE> and stage_to_lds) and the
    peeled last tile, on non-integer inputs."""
    ntaps, M, fp = case
    T, chunk = cf32_geometry(M)
    assert T == {1: 4096, 2: 4096, 3: 6144, 6: 6144, 12: 6144, 4: 8192, 8: 8192, 16: 8192}[M]
    calls = call_pattern(T, M, chunk, ntaps)
    c = cf32_taps(ntaps, M)
    x = O[fp].gen_cf32(0x100B + ntaps, M, 0, sum(calls), -32768, 32767) + np.float32(0.37)
    g, r = cf32_filter(S, O, c, M, fp)
    hist = History(ntaps - 1, x)

    def after(k, xs, what):
        hist.push(xs)
        if M > 1:
            hist.check(g, what)

    cap(cap_n)
    drive(S, cap_n, T, calls, x, "cf32", g.step, r.step, after)


@pytest.mark.parametrize("M", CF32_RT_M)
def test_cf32_tile_loop_shifted_quantiser(S, O, cap, M):
    """The Q0 = false instantiations: (shift & 31) != 0 is what the
    constructor leaves for taps whose magnitudes sum to 2 or more
    (coeffScaling = floor(log2(sum |c|)) >= 1), and what setLeftShiftBy2 makes
    of any filter; both are used here (the fabs binding at even M, the
    canonical integer one at odd M; M = 1 is FilterFir, which has no left
    shift)."""
    ntaps, fp = 100, ("fma" if M in (1, 4, 12) else "strict")
    T, chunk = cf32_geometry(M)
    calls = call_pattern(T, M, chunk, ntaps)
    rng = np.random.default_rng(4242 + M)
    c = (rng.standard_normal(ntaps) * 3.0).astype(np.float32)
    binding = "fabs" if M % 2 == 0 else "int"
    g, r = cf32_filter(S, O, c, M, fp, binding)
    if M > 1:
        g.setLeftShiftBy2(1)
        r.set_left_shift(1)
        st = g.state()
        assert st["coeff_scaling"] == r.coeff_scaling and st["left_shift"] == 1
        assert ((st["coeff_scaling"] - 1) & 31) != 0
    else:  # sum |c| of 100 taps of deviation 3 is far above 2 under either binding
        assert np.abs(np.trunc(c)).sum() >= 64
    x = O[fp].gen_cf32(0x5111 + M, M, 0, sum(calls), -32768, 32767) + np.float32(0.37)
    cap(16)
    drive(S, 16, T, calls, x, "cf32", g.step, r.step)


# ================================================================== decim_dot2_ci16
def dot2_T(M):
    return 4096 if M == 1 else 8192   # 16 samples per lane; 256 lanes at M = 1, else 512


def dot2_taps(ntaps, M):
    rng = np.random.default_rng(2000 + 7 * M + ntaps)
    c = rng.integers(-32768, 32768, size=ntaps).astype(np.int32)
    c[0], c[-1] = 32767, -32768
    return c


# (ntaps, M): compiled at M = 4 x 63/64/127/128/255/256; 200, 100 and 31 taps take the runtime kernel
DOT2_UNMIXED = [(63, 4), (64, 4), (127, 4), (128, 4), (255, 4), (256, 4), (200, 4),
                (100, 1), (200, 2), (1024, 8), (31, 16)]
DOT2_UNMIXED_PARAMS = with_caps(DOT2_UNMIXED, [(127, 4), (100, 1)])


@pytest.mark.parametrize("cap_n,case", DOT2_UNMIXED_PARAMS, ids=ids(DOT2_UNMIXED_PARAMS))
def test_dot2_tile_loop(S, O, cap, cap_n, case):
    """decim_dot2_ci16 unmixed: the per/rem split of [t_begin, t_end) and
    stage_load(tile + 1), full-scale inputs and int16-extreme taps."""
    ntaps, M = case
    T = dot2_T(M)
    calls = call_pattern(T, M, 16, ntaps)
    c = dot2_taps(ntaps, M)
    x = O["strict"].gen_ci16(0xD072 + ntaps, M, 0, sum(calls), -32768, 32767)
    g, r = S.FilterDnsamplingFir(c, M, *CI16), O["strict"].decim(1, M, c)
    hist = History(ntaps - 1, x)

    def after(k, xs, what):
        hist.push(xs)
        hist.check(g, what)

    cap(cap_n)
    drive(S, cap_n, T, calls, x, "ci16", g.step, r.step, after)


# ---- the fused mixer's table forms: the rules of decim.hip, restated
def mixer_seq_period(N, fr):
    """lcm(N / gcd(freq, N), 4): the period of the table index over input samples."""
    P = N // math.gcd(fr, N)
    return P if P % 4 == 0 else (2 * P if P % 2 == 0 else 4 * P)


def dot2_mixer_form(ntaps, M, N, fr):
    """launch_ci16_dot2: the table form a mixed call takes."""
    block = 256 if M == 1 else 512
    runtime = not (M == 4 and ntaps in (127, 128))
    pe = mixer_seq_period(N, fr)
    if pe > 4096:
        return 1
    if block == 512 and not (runtime and M == 2) and (16 * block) % pe == 0:
        return 5
    return 3 if pe <= 2048 else 4


# form -> (N, f, the frequency after the retune), each pair of the form's own
# class: 1: Pe > 4096 (N = 4093 is prime: Pe = 4 N); 5: Pe | 8192 at 512 lanes
# (N = 4096, an odd word: Pe = 4096); 3: Pe <= 2048, not dividing 8192 (N = 1022:
# words 460 and 189, Pe = 2044 and 292); 4: 2048 < Pe <= 4096, not dividing 8192
# (N = 3000, words 451 and 151 coprime to it: Pe = 3000).  Where form 5 is not
# compiled (256 lanes at M = 1; runtime taps at M = 2) N = 4096 takes form 4.
FORM_MIXERS = {1: (4093, 0.1, -0.2), 5: (4096, 0.1, 0.73), 3: (1022, 0.9, 0.37), 4: (3000, 0.3007, 0.1007),
               "4p": (4096, 0.1, 0.73)}
DOT2_MIXED_SHAPES = [(127, 4), (128, 4), (200, 4), (100, 1), (200, 2), (1024, 8), (31, 16)]


def forms_of(ntaps, M):
    if M in (1, 2):                  # launch_ci16_dot2<0, 1> (256 lanes) and <0, 2>: no form 5
        return [1, 3, 4, "4p"]
    return [1, 3, 4, 5]


DOT2_MIXED = [(n, M, f) for n, M in DOT2_MIXED_SHAPES for f in forms_of(n, M)]
DOT2_MIXED_PARAMS = with_caps(DOT2_MIXED, [(127, 4, 1), (127, 4, 3), (127, 4, 4), (127, 4, 5), (100, 1, "4p")])


def mixed_chain_case(S, O, cap, cap_n, ntaps, M, T, c, N, f, f2, form_of=None):
    """A MixerDecimatorChain over the call pattern with a retune after the
    third call: outputs, mixer state and decimator history after every call."""
    calls = call_pattern(T, M, 16, ntaps)
    x = O["strict"].gen_ci16(0x3177 + ntaps + N, M, 0, sum(calls), -32768, 32767)
    m = S.Mixer(N)
    m.reset(f)
    d = S.FilterDnsamplingFir(c, M, *CI16)
    chain = S.MixerDecimatorChain(m, d)
    om, od = O["strict"].mixer(N), O["strict"].decim(1, M, c)
    om.reset(f)
    hist = History(ntaps - 1, x)
    forms = []

    def ref_step(xs):
        forms.append(form_of(m.state()[1]) if form_of else None)
        ref_step.mixed = om.step(xs)
        return od.step(ref_step.mixed)

    def after(k, xs, what):
        assert m.state()[:2] == om.state()[:2], what
        hist.push(ref_step.mixed)
        hist.check(d, what)
        if k == 2:  # a retune between two calls: the phase carries, the word changes
            m.setFrequency(f2)
            om.set_frequency(f2)
            assert m.state()[:2] == om.state()[:2] and m.state()[1] != 0

    cap(cap_n)
    drive(S, cap_n, T, calls, x, "ci16", chain.step, ref_step, after)
    return forms


@pytest.mark.parametrize("cap_n,case", DOT2_MIXED_PARAMS, ids=ids(DOT2_MIXED_PARAMS))
def test_dot2_mixed_tile_loop(S, O, cap, cap_n, case):
    """decim_dot2_ci16 with the mixer fused, every table form its launcher can
    select: tile_phase(tile) per tile (form 1), m_tile = advp(m_tile,
    mix_pe_dtile) (forms 3 and 4), the register words (form 5); the workgroup
    that stages tile 0 from the history goes on to tile 1 from memory."""
    from srcdsp_amd.design import hamming_sinc, q14
    ntaps, M, form = case
    want_form = 4 if form == "4p" else form
    N, f, f2 = FORM_MIXERS[form]
    c = q14(hamming_sinc(ntaps))
    forms = mixed_chain_case(S, O, cap, cap_n, ntaps, M, dot2_T(M), c, N, f, f2,
                             lambda fr: dot2_mixer_form(ntaps, M, N, fr))
    assert forms == [want_form] * 5, forms   # the form that served every call, the retuned ones included


def test_mixer_forms_meet_the_periods_the_rule_needs(S):
    """The (N, f) above give the periods their forms need, with the frequency
    words the mixer itself makes of them."""
    for form, (N, f, f2) in FORM_MIXERS.items():
        for fq in (f, f2):
            m = S.Mixer(N)
            m.reset(fq)
            pe = mixer_seq_period(N, m.state()[1])
            if form == 1:
                assert pe > 4096
            elif form == 5 or form == "4p":
                assert pe <= 4096 and 8192 % pe == 0 and pe > 2048
            elif form == 3:
                assert pe <= 2048 and 8192 % pe != 0 and 4096 % pe != 0
            else:
                assert 2048 < pe <= 4096 and 8192 % pe != 0
    assert mixer_seq_period(4096, 0) == 4 and mixer_seq_period(1022, 460) == 2044


# ================================================================ decim_stream_ci16
CI16_STREAM = [(127, False), (128, False), (127, True), (128, True)]
CI16_STREAM_PARAMS = with_caps(CI16_STREAM, [(127, True)])


@pytest.mark.parametrize("cap_n,case", CI16_STREAM_PARAMS, ids=ids(CI16_STREAM_PARAMS))
def test_ci16_stream_tile_loop(S, O, cap, cap_n, case):
    """decim_stream_ci16<127|128>: taps with |c| < 2^23 that do not fit int16,
    unmixed and with the mixer fused (stage_mix(tile) at tile_phase(tile))."""
    ntaps, mixed = case
    rng = np.random.default_rng(900 + ntaps)
    c = rng.integers(-(1 << 23) + 1, 1 << 23, size=ntaps).astype(np.int32)
    c[0], c[-1], c[ntaps // 2] = (1 << 23) - 1, -(1 << 23) + 1, 40000
    assert 32768 < np.abs(c).max() < 1 << 23
    T = 4096
    if mixed:
        mixed_chain_case(S, O, cap, cap_n, ntaps, 4, T, c, 1000, -0.37, 0.3)
        return
    calls = call_pattern(T, 4, 16, ntaps)
    x = O["strict"].gen_ci16(0xC116 + ntaps, 4, 0, sum(calls), -32768, 32767)
    g, r = S.FilterDnsamplingFir(c, 4, *CI16), O["strict"].decim(1, 4, c)
    hist = History(ntaps - 1, x)

    def after(k, xs, what):
        hist.push(xs)
        hist.check(g, what)

    cap(cap_n)
    drive(S, cap_n, T, calls, x, "ci16", g.step, r.step, after)


# =================================================================== fir_stream_f32
FIR_CASES = [(n, fp) for n in (31, 5, 128) for fp in ("fma", "strict")]
FIR_PARAMS = with_caps(FIR_CASES, [(31, "fma"), (128, "strict")])


@pytest.mark.parametrize("cap_n,case", FIR_PARAMS, ids=ids(FIR_PARAMS))
def test_fir_stream_tile_loop(S, O, cap, cap_n, case):
    """fir_stream_f32 (float in, complex<float> out): 31 taps compiled in and
    the runtime loop at 5 and at 128 taps (the longest the stream kernel takes)."""
    ntaps, fp = case
    T = 2048
    calls = call_pattern(T, 1, 8, ntaps)
    rng = np.random.default_rng(ntaps)
    c = (rng.standard_normal(ntaps) / max(4, ntaps)).astype(np.float32)
    x = O[fp].gen_cf32(0xF1F + ntaps, 0, 0, sum(calls), -32768, 32767).real.astype(np.float32) + np.float32(0.37)
    g = S.FilterFir(c, "float", "complex<float>", "float", "float", fp=fp)
    r = O[fp].fir(1, c)
    cap(cap_n)
    drive(S, cap_n, T, calls, x, "cf32", g.step, r.step)


# ==================================================================== ddc_bank_ci16
BANK_T = 4096


def bank_group(nc, ntiles, shared, cap_n):
    """bank_launch: channels per workgroup.  On a shared input, up to 8, halved
    while the grid would fill less than half of the (capped) 2048 workgroups."""
    eff = min(2048, cap_n) if cap_n else 2048
    g = 1
    if shared:
        g = min(8, nc)
        while g > 1 and ntiles * -(-nc // g) < eff // 2:
            g = (g + 1) // 2
    return g, max(1, eff // -(-nc // g))   # and the workgroups in x the launch may use


def bank_calls(ntaps):
    """The call pattern at M = 4 with the bank suite's own short calls (32
    samples: under a lane chunk pair; 100: shorter than a 126-sample history)
    and two calls short enough to shrink the group."""
    assert CHUNKS[1:3] == [32, 100]
    return [37 * BANK_T + 12, CHUNKS[1], min(CHUNKS[2], short_call(ntaps, 4)), 9 * BANK_T, 20 * BANK_T,
            5 * BANK_T, 3 * BANK_T]


_BANK_X, _BANK_REF = {}, {}


def bank_signal(O, ch, n):
    if (ch, n) not in _BANK_X:
        _BANK_X[(ch, n)] = O["strict"].gen_ci16(0xDDC, ch, 0, n, -32768, 32767)
    return _BANK_X[(ch, n)]


def bank_reference(O, ch, ntaps, f, calls):
    """Per call: the oracle's outputs, mixer state and decimator history for
    input channel ch through a mixer at f; made once per (input, filter, f)."""
    k = (ch, ntaps, f, tuple(calls))
    if k not in _BANK_REF:
        cq = bank_taps(ntaps)
        om, od = O["strict"].mixer(4096), O["strict"].decim(1, 4, cq)
        om.reset(f)
        x = bank_signal(O, ch, sum(calls))
        hist = History(ntaps - 1, x)
        outs, states, hists, off = [], [], [], 0
        for n in calls:
            mixed = om.step(x[off:off + n])
            off += n
            outs.append(od.step(mixed))
            states.append(om.state()[:2])
            hist.push(mixed)
            hists.append(np.ascontiguousarray(hist.buf).tobytes())
        _BANK_REF[k] = (outs, states, hists)
    return _BANK_REF[k]


BANK_CASES = [("shared", 8, 1), ("shared", 8, 31), ("shared", 8, 127), ("shared", 8, 1024), ("shared", 11, 127),
              ("shared", 64, 31), ("rows", 8, 127)]
BANK_PARAMS = with_caps(BANK_CASES, [("shared", 8, 127), ("shared", 11, 127)])


@pytest.mark.parametrize("cap_n,case", BANK_PARAMS, ids=ids(BANK_PARAMS))
def test_bank_channel_groups_and_tile_loop(S, O, cap, cap_n, case):
    """ddc_bank_ci16 with group > 1 and several tiles per workgroup: one fetch
    of a tile mixed for up to 8 channels, the next tile's loads issued after
    the group's last channel, a partial last group (11 = 8 + 3 channels), 64
    channels, and one input row per channel (group 1, several tiles)."""
    from srcdsp_amd import _capi as A
    layout, nc, ntaps = case
    shared = layout == "shared"
    calls = bank_calls(ntaps)
    total = sum(calls)
    cq = bank_taps(ntaps)
    ms, ds = [], []
    for c in range(nc):
        m = S.Mixer(4096)
        m.reset(FREQS[c % len(FREQS)])
        ms.append(m)
        ds.append(S.FilterDnsamplingFir(cq, 4, *CI16))
    hm = (C.c_void_p * nc)(*[m._h.value for m in ms])
    hd = (C.c_void_p * nc)(*[d._h.value for d in ds])
    refs = [bank_reference(O, 0 if shared else c, ntaps, FREQS[c % len(FREQS)], calls) for c in range(nc)]
    x = bank_signal(O, 0, total) if shared else np.stack([bank_signal(O, c, total) for c in range(nc)])
    groups = []
    cap(cap_n)
    off = 0
    for k, n in enumerate(calls):
        group, xgrid = bank_group(nc, tiles(n, BANK_T), shared, cap_n)
        groups.append(group)
        xd = dev(x[off:off + n] if shared else x[:, off:off + n])
        off += n
        n_out = n // 4
        stride = (n_out + GUARD + 3) // 4 * 4
        buf = poisoned("ci16", n_out, nc, stride)
        b0, lp0 = S.mixdecim_batched_stats()
        a0, l0 = S.stream_grid_stats()
        A.call("srcdsp_mixdecim_step_batched", hm, hd, nc, C.c_void_p(xd.data_ptr()), 0 if shared else n,
               C.c_void_p(buf.data_ptr()), stride, n, stream_ptr())
        a1, l1 = S.stream_grid_stats()
        b1, lp1 = S.mixdecim_batched_stats()
        what = f"call {k} of {n} samples ({tiles(n, BANK_T)} tiles, group {group}, {xgrid} workgroups in x)"
        assert (b1 - b0, lp1 - lp0) == (1, 0), what   # the bank kernel served it
        assert (a1 - a0, l1 - l0) == (1, int(tiles(n, BANK_T) > xgrid)), what
        check_rows(buf, "ci16", n_out, [r[0][k] for r in refs], what)
        for c in range(nc):
            assert ms[c].state()[:2] == refs[c][1][k], (what, c)
            if ntaps > 1:
                assert ds[c].state()["history"].tobytes() == refs[c][2][k], (what, c)
    if cap_n == 16 and shared and nc == 8:
        assert groups == [8, 1, 1, 8, 8, 4, 2], groups
    if cap_n == 16 and shared and nc == 11:
        assert groups == [8, 1, 1, 8, 8, 8, 4], groups   # groups of 8 and 3, then 4, 4 and 3
    if not shared:
        assert groups == [1] * len(calls)


# ======================================================== srcdsp_decim_step_batched
BATCHED = ["cf32", "dot2"]
BATCHED_PARAMS = with_caps([(b,) for b in BATCHED], [("cf32",)])


@pytest.mark.parametrize("cap_n,case", BATCHED_PARAMS, ids=ids(BATCHED_PARAMS))
def test_batched_decimator_tile_loop(S, O, cap, cap_n, case):
    """3 channels in one launch (grid.y = channel) at one cf32 and one dot2
    shape: the cap bounds grid.x, every row loops on its own tiles."""
    from srcdsp_amd import _capi as A
    from srcdsp_amd.design import hamming_sinc
    kind = case[0]
    nc, M, ntaps, T = 3, 4, 127, 8192
    calls = call_pattern(T, M, 16, ntaps)
    total = sum(calls)
    if kind == "cf32":
        c = hamming_sinc(ntaps)
        x = np.stack([O["fma"].gen_cf32(0xBA7, ch, 0, total, -32768, 32767) + np.float32(0.37) for ch in range(nc)])
        fs = [S.FilterDnsamplingFir(c, M) for _ in range(nc)]
        rs = [O["fma"].decim(0, M, c) for _ in range(nc)]
        okind, quantum = "cf32", 2
    else:
        c = dot2_taps(ntaps, M)
        x = np.stack([O["strict"].gen_ci16(0xBA7, ch, 0, total, -32768, 32767) for ch in range(nc)])
        fs = [S.FilterDnsamplingFir(c, M, *CI16) for _ in range(nc)]
        rs = [O["strict"].decim(1, M, c) for _ in range(nc)]
        okind, quantum = "ci16", 4
    hs = (C.c_void_p * nc)(*[f._h.value for f in fs])
    hists = [History(ntaps - 1, x[ch]) for ch in range(nc)]
    cap(cap_n)
    off = 0
    for k, n in enumerate(calls):
        xs = x[:, off:off + n]
        off += n
        n_out = n // M
        stride = (n_out + GUARD + quantum - 1) // quantum * quantum   # rows stay 16-byte aligned
        buf = poisoned(okind, n_out, nc, stride)
        xd = dev(xs)
        a0, l0 = S.stream_grid_stats()
        A.call("srcdsp_decim_step_batched", hs, nc, C.c_void_p(xd.data_ptr()), n, C.c_void_p(buf.data_ptr()),
               stride, n, stream_ptr())
        a1, l1 = S.stream_grid_stats()
        what = f"call {k} of {n} samples ({tiles(n, T)} tiles, cap {cap_n})"
        assert (a1 - a0, l1 - l0) == (1, int(tiles(n, T) > cap_n)), what
        check_rows(buf, okind, n_out, [rs[ch].step(xs[ch]) for ch in range(nc)], what)
        for ch in range(nc):
            hists[ch].push(xs[ch])
            hists[ch].check(fs[ch], (what, ch))


# ============================================================ the cap is put back
def test_zz_cap_is_zero_again_and_an_uncapped_call_does_not_loop(S, O):
    """Last in the module: every test above left the product grids in place,
    and under them a 4-tile call is 4 workgroups of one tile."""
    from srcdsp_amd.design import hamming_sinc
    assert S.stream_get_grid_cap() == 0
    c = hamming_sinc(127)
    x = O["fma"].gen_cf32(0x5EED, 0, 0, 4 * 8192)
    g, r = S.FilterDnsamplingFir(c, 4), O["fma"].decim(0, 4, c)
    want = r.step(x)
    buf = poisoned("cf32", len(want))
    a0, l0 = S.stream_grid_stats()
    g.step(dev(x), buf[0, :len(want)])
    a1, l1 = S.stream_grid_stats()
    assert (a1 - a0, l1 - l0) == (1, 0)
    check_rows(buf, "cf32", len(want), [want], "uncapped 4-tile call")
