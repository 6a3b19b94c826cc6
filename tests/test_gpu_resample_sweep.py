"""Every instantiation and edge of the interpolator -> decimator tile
(resample_tile_dot2, resample_kernels.h) against the oracle's two calls.  The
launcher (resample.hip) dispatches on (L, PP = ceil(H / 2)), H taps per phase,
to 10 kernels: PP compiled in at (L, PP) = (2,16) (4,16) (8,8), H at run time
at L = 2..8.  The shapes (L, H, M, N_d) below name them all:

    COMPILED  (2,32,5,8) (4,32,7,9) (8,16,3,7): the three kernels; (2,31,8,1023)
              (4,31,2,2) (8,15,6,1024): the same PP with a padded last pair
    RUNTIME   one per L = 2..8 and more: H = 1 (no interpolator history), N_d = 1
              (no decimator history), M = 1 at the N_d cap
    CEILING   (8,512,7,1024): kUpMaxTaps and kRsMaxDecimTaps, the largest LDS
              launch; (2,2048,7,1024): the input planes staged 8 HG = 2568
              samples ahead of a tile, deeper than a tile, so tile 1 stages from
              before the stream's start; (8,512,8,1023): an even M there

With the shapes of test_gpu_resample.py every M = 1..8 meets an even and an odd
L, and N_d stands on both sides of every step of rs_halo_words and
rs_decim_pairs4 (resample_index.h) below 17; test_the_sweep_covers_what_it_names
derives that from the lists by the launcher's rule.

Two kinds of taps.  "full" is test_gpu_resample.py's: random full-range int16
taps and full-scale input at the smallest left shift that puts 10-95 % of the
oracle's outputs on +-32767, which pins the int32 wrap, both clamps and their
order.  "dense" has every tap non-zero and the end taps at full size, moderate
input, and the largest interpolator amplitude and decimator left shift at which
under 1 % of the oracle's samples sit on a clamp: every low bit of every output
shows, and a halo or a tap table one word short changes the outputs (the
reference itself notices an end tap going missing:
test_the_dense_reference_sees_every_end_tap).

Every case is one chain over the call plan of test_gpu_resample.py (two tiles
and a ragged third, one lane, fewer inputs than the history, L n < N_d - 1, one
tile, a flushing rest); after every call the output equals the oracle's, both
handles' state equals twin handles stepped through the single operators, the
counters rose by exactly one on the fused path and the 24 samples behind the
output keep their fill value.  Banks of 3 rows with their own inputs and
histories, flushing, every row against its own oracle chain."""
import math

import numpy as np
import pytest

import test_gpu_resample as R
from test_gpu_resample import BANK, FUSED, LOOP, handles, oracle_chain, same_state, shape_calls
from test_gpu_upmix import dev, signal

gpu = pytest.mark.gpu

# (L, H, M, N_d)
COMPILED = [(2, 32, 5, 8), (4, 32, 7, 9), (8, 16, 3, 7), (2, 31, 8, 1023), (4, 31, 2, 2), (8, 15, 6, 1024)]
RUNTIME = [(2, 5, 7, 1), (3, 9, 7, 3), (4, 3, 5, 16), (5, 7, 4, 6), (5, 2, 3, 33), (6, 1, 7, 8), (7, 11, 5, 17),
           (8, 33, 1, 5), (3, 9, 1, 1024)]
CEILING = [(8, 512, 7, 1024), (2, 2048, 7, 1024), (8, 512, 8, 1023)]
SHAPES = COMPILED + RUNTIME + CEILING
BANK_SHAPES = [(8, 16, 3, 7), (5, 7, 4, 6)]
LOOP_SHAPE = (4, 32, 3, 96)
KINDS = ("full", "dense")
GUARD = 24
TILE, MAX_UP_TAPS, MAX_DECIM_TAPS = 2048, 4096, 1024


@pytest.fixture(scope="module")
def fused_on_every_shape_it_takes(S):
    yield from R.force_fused(S)


# ------------------------------------------- the index functions of resample_index.h
def rs_halo_words(Nd):
    return (Nd + 1 + 7) & ~7


def rs_decim_pairs4(Nd):
    return (Nd // 2 + 1 + 3) & ~3


def rs_halo_granules(PP, L, HP):
    return (2 * PP + (HP + L - 1) // L + 7) // 8


def rs_planes_bytes(HG):
    return 4 * 4 * 4 * (TILE // 8 + HG)


def rs_mid_bytes(L, HP):
    return 8 * (HP // 2 + L * TILE // 2 + 2)


def rs_smem(H, L, Nd):
    HP = rs_halo_words(Nd)
    return rs_planes_bytes(rs_halo_granules((H + 1) // 2, L, HP)) + rs_mid_bytes(L, HP) + 8 * rs_decim_pairs4(Nd)


def kernel_of(L, H):
    """The instantiation <LR, PPC> fused_launch (resample.hip) picks."""
    PP = (H + 1) // 2
    return (L, PP) if (L, PP) in ((2, 16), (4, 16), (8, 8)) else (L, 0)


def test_the_index_port_gives_the_header_comments_numbers():
    """resample_kernels.h: HP = 1032 halo words at the cap; rs_smem(512, 8, 1024)
    = 21 568 B of planes + 69 680 B of mid plane + 4128 B of tap pairs = 95 376 B."""
    HP = rs_halo_words(MAX_DECIM_TAPS)
    assert HP == 1032 and 4 * HP == 4128
    HG = rs_halo_granules(256, 8, HP)
    assert (rs_planes_bytes(HG), rs_mid_bytes(8, HP), 8 * rs_decim_pairs4(MAX_DECIM_TAPS)) == (21568, 69680, 4128)
    assert rs_smem(512, 8, 1024) == 95376 <= 160 * 1024
    # the pairs walked four at a time end where the halo starts: HP / 2 = rs_decim_pairs4 (resample_index.h)
    assert all(rs_halo_words(n) // 2 == rs_decim_pairs4(n) for n in range(1, MAX_DECIM_TAPS + 1))


def test_the_sweep_covers_what_it_names():
    assert all(2 <= L <= 8 and L * H <= MAX_UP_TAPS and 1 <= M <= 8 and Nd <= MAX_DECIM_TAPS for L, H, M, Nd in SHAPES)
    # all 10 kernels, the compiled ones with a whole and with a padded last pair
    assert {kernel_of(L, H) for L, H, _, _ in SHAPES} == {(2, 16), (4, 16), (8, 8)} | {(L, 0) for L in range(2, 9)}
    assert {kernel_of(L, H) for L, H, _, _ in COMPILED} == {(2, 16), (4, 16), (8, 8)}
    assert {(kernel_of(L, H), H % 2) for L, H, _, _ in COMPILED} == {(k, p) for k in ((2, 16), (4, 16), (8, 8))
                                                                      for p in (0, 1)}
    assert all(kernel_of(L, H)[1] == 0 for L, H, _, _ in RUNTIME + CEILING)
    # every M with an even and with an odd L, the shapes of test_gpu_resample.py counted in
    pairs = {(L, M) for L, _, M, _ in SHAPES} | {(L, M) for L, _, M, _ in R.SHAPES}
    for M in range(1, 9):
        assert {L % 2 for L, m in pairs if m == M} == {0, 1}, M
    assert any(L % 2 and M in (3, 5, 7) for L, M in pairs)
    # N_d on both levels of every step of the halo and of the tap table below 17
    nds = {Nd for _, _, _, Nd in SHAPES}
    assert nds >= {1, 2, 3, 5, 6, 7, 8, 9, 16, 17, 33, 1023, 1024}
    for f in (rs_halo_words, rs_decim_pairs4):
        steps = [n for n in range(2, 17) if f(n) != f(n - 1)]
        assert steps == [8, 16], (f.__name__, steps)
        for s in steps:
            assert {f(s - 1), f(s)} <= {f(n) for n in nds}, (f.__name__, s)
            assert s in nds  # the first N_d of the new level itself
    assert 7 in nds  # and the last of the first
    # the ceiling: the largest LDS launch, and planes staged deeper than a tile
    (L0, H0, _, Nd0), (L1, H1, _, Nd1) = CEILING[:2]
    assert rs_smem(H0, L0, Nd0) == 95376 == max(rs_smem(H, L, Nd) for L, H, _, Nd in SHAPES)
    assert 8 * rs_halo_granules((H1 + 1) // 2, L1, rs_halo_words(Nd1)) == 2568 > TILE
    assert CEILING[2][2] % 2 == 0 and CEILING[2][0] * CEILING[2][1] == MAX_UP_TAPS
    # the call plan of every shape: three tiles first, then the short calls it is cut for
    for L, H, M, Nd in SHAPES:
        calls, total = shape_calls(L, L * H, M)
        ns = [n for _, n, _ in calls]
        assert 2 * TILE < ns[0] <= 3 * TILE and ns[0] % TILE and calls[-1][2] and 8900 <= total <= 9100
        if Nd > 300:
            assert any(L * n < Nd - 1 for n in ns), (L, H, M, Nd)
        if H > 40:
            assert any(n < H - 1 for n in ns), (L, H, M, Nd)


# ---------------------------------------------------------------- the two kinds of taps
def dense_taps(seed, n, A):
    """n taps uniform in +-A, none zero, c[0] = A and (n >= 2) c[-1] = -A."""
    rng = np.random.default_rng(seed)
    c = (rng.integers(1, A + 1, n) * rng.choice([-1, 1], n)).astype(np.int32)
    c[-1] = -A
    c[0] = A
    return c


def on_clamp(y):
    y = np.concatenate(y).astype(np.int32)
    return float(np.mean((y >= 32767) | (y <= -32767)))


_DENSE = {}


def dense_parts(O, L, H, M, Nd):
    """(cu, cd, ls) of a dense case, searched on the oracle alone: A, the
    interpolator taps' amplitude, is the largest power of two <= 16384 that
    leaves under 1 % of the oracle's interpolated samples on a clamp (and, where
    the decimator has so few taps that it clamps at left shift 0, under 1 % of
    its outputs there); the left shift is the largest that leaves under 1 % of
    the oracle's outputs on the clamp (the decimator over the stored
    interpolator output)."""
    key = (L, H, M, Nd)
    if key not in _DENSE:
        o = O["strict"]
        Nu = L * H
        calls, total = shape_calls(L, Nu, M)
        x = signal(O, "sinc", 0, total + 8)
        cd = dense_taps(6000 + 10000 * M + Nd, Nd, 32767)

        def decimate(ls):
            dec = o.decim(1, M, cd)
            dec.set_left_shift(ls)
            return [dec.step(m) for m in mids]

        A = 2 * 16384
        while True:
            A //= 2
            assert A >= 2, "no amplitude keeps both filters off their clamps"
            cu = dense_taps(5000 + 100 * L + H, Nu, A)
            up = o.up(0, L, cu)
            mids = [up.step(x[off:off + n], last) for off, n, last in calls]
            mid_share = on_clamp(mids)
            if mid_share >= 0.01:
                continue
            ls, outs = 0, decimate(0)
            if on_clamp(outs) < 0.01:  # else: the decimator clamps without any left shift (few taps), a smaller A
                break
        while ls < 15:
            more = decimate(ls + 1)
            if on_clamp(more) >= 0.01:
                break
            ls, outs = ls + 1, more
        share = on_clamp(outs)
        rms = float(np.sqrt(np.mean(np.concatenate(outs).astype(np.float64) ** 2)))
        print(f"dense {key}: A {A}, share of mid on a clamp {mid_share:.4f}, left shift {ls}, "
              f"share of outputs on the clamp {share:.4f}, output rms {rms:.0f}")
        assert mid_share < 0.01 and share < 0.01 and rms > 1000, (A, mid_share, ls, share, rms)
        _DENSE[key] = (cu, cd, ls)
    return _DENSE[key]


def sweep_reference(O, kind, L, H, M, Nd):
    if kind == "full":
        return R.reference(O, "full", L, L * H, M, Nd)
    cu, cd, ls = dense_parts(O, L, H, M, Nd)
    return R.reference(O, "dense", L, L * H, M, Nd, cu=cu, cd=cd, ls=ls)


def ident(shape):
    return "L{}xH{}-M{}-Nd{}".format(*shape)


@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_the_dense_reference_sees_every_end_tap(O, shape):
    """A condition on the reference, not on the kernel: a tile that lost the
    oldest or the newest tap of either filter could not pass the dense case.
    The oldest interpolator tap is negated, not zeroed: a zero tail shortens
    the filter's length, and with it the flush."""
    L, H, M, Nd = shape
    ref = sweep_reference(O, "dense", L, H, M, Nd)
    want = np.concatenate(ref["outs"])

    def changed(cu, cd):
        y = np.concatenate(oracle_chain(O, ref["x"], ref["calls"], 0, L, cu, 1, M, cd, ref["ls"]))
        assert y.shape == want.shape
        return float(np.mean((y != want).any(1)))

    def with_tap(c, k, v):
        c = c.copy()
        c[k] = v
        return c

    cu, cd = ref["cu"], ref["cd"]
    shares = dict(cd_first_negated=changed(cu, with_tap(cd, 0, -cd[0])),
                  cu_first_zeroed=changed(with_tap(cu, 0, 0), cd),
                  cu_last_negated=changed(with_tap(cu, -1, -cu[-1]), cd))
    if Nd >= 2:
        shares["cd_last_zeroed"] = changed(cu, with_tap(cd, Nd - 1, 0))
    print(f"dense {shape}: share of outputs changed " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares["cd_first_negated"] >= 0.90 and shares.get("cd_last_zeroed", 1.0) >= 0.90, shares
    assert shares["cu_first_zeroed"] >= 0.40 and shares["cu_last_negated"] >= 0.40, shares


# ------------------------------------------------------------------ the sweep
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_instantiation_vs_oracle(S, O, fused_on_every_shape_it_takes, shape, kind):
    L, H, M, Nd = shape
    R.run_and_check(S, sweep_reference(O, kind, L, H, M, Nd), L, M, FUSED, guard=GUARD)


# -------------------------------------------------------------------- banks
ROWS = 3


def bank_plan(L, H, M):
    """(first calls of the rows, the batched call of two tiles, the short flushing one)."""
    g = M // math.gcd(L, M)
    n0 = [24 * (r + 1) for r in range(ROWS)]
    n1 = 2055 // g * g
    n2 = 7 + (-(7 + H)) % g
    assert all(n % g == 0 for n in n0) and n1 > TILE and (n2 + H) % g == 0
    return n0, n1, n2


def run_bank(S, O, shape, want, in_pad):
    import torch
    L, H, M, Nd = shape
    cu, cd, ls = dense_parts(O, L, H, M, Nd)
    ref = dict(cu=cu, cd=cd, ls=ls)
    n0, n1, n2 = bank_plan(L, H, M)
    xs = [signal(O, "sinc", 1 + r, n0[r] + n1 + n2) for r in range(ROWS)]
    wants = [oracle_chain(O, xs[r], [(0, n0[r], False), (n0[r], n1, False), (n0[r] + n1, n2, True)], 0, L, cu, 1, M,
                          cd, ls) for r in range(ROWS)]
    pairs = [handles(S, ref, L, M) for _ in range(ROWS)]
    twins = [handles(S, ref, L, M) for _ in range(ROWS)]
    probe = dev(xs[0][:64])
    for r in range(ROWS):  # every row its own histories, by a single call
        for up, dec in (pairs[r], twins[r]):
            y = S.RationalResampler(up, dec).step(dev(xs[r][:n0[r]]))
            assert np.array_equal(y.cpu().numpy(), wants[r][0]), r
    ups, decs = [p[0] for p in pairs], [p[1] for p in pairs]
    for k, (n, flush) in enumerate(((n1, False), (n2, True))):
        stride = (n + 3) // 4 * 4 + in_pad
        host = np.zeros((ROWS, stride, 2), np.int16)
        for r in range(ROWS):
            off = n0[r] + (n1 if k else 0)
            host[r, :n] = xs[r][off:off + n]
        x = dev(host)[:, :n]
        assert (x.stride(0) * 2) % 16 == (0 if in_pad == 0 else 4 * in_pad)
        n_out = len(wants[0][1 + k])
        out = torch.full((ROWS, (n_out + GUARD + 3) // 4 * 4, 2), R.GUARD_VALUE, dtype=torch.int16, device="cuda")
        s0 = S.resample_stats()
        S.resample_step_batched(ups, decs, x, out, flush)
        d = tuple(b - a for a, b in zip(s0, S.resample_stats()))
        assert d == tuple(int(i == want) for i in range(4)), (k, d)
        y = out.cpu().numpy()
        assert (y[:, n_out:] == R.GUARD_VALUE).all(), k
        for r in range(ROWS):
            assert np.array_equal(y[r, :n_out], wants[r][1 + k]), (k, r)
            tup, tdec = twins[r]
            off = n0[r] + (n1 if k else 0)
            yt = tdec.step(tup.step(dev(xs[r][off:off + n]), None, flush))
            assert np.array_equal(yt.cpu().numpy(), wants[r][1 + k]), (k, r)
            same_state(S, ups[r], decs[r], tup, tdec, ls, probe, (k, r))


@gpu
@pytest.mark.parametrize("shape", BANK_SHAPES, ids=ident)
def test_bank_vs_oracle(S, O, fused_on_every_shape_it_takes, shape):
    run_bank(S, O, shape, BANK, 0)


@gpu
def test_bank_with_an_input_row_stride_off_16_bytes_flushes_through_the_loop(S, O, fused_on_every_shape_it_takes):
    run_bank(S, O, LOOP_SHAPE, LOOP, 2)
