"""srcdsp_freqest_* on the GPU against tests/freqest_model.py: the sums exactly,
the float bit for bit, `exact` equal.  T is the kernel's tile in pairs, W its
vector width in samples, G the persistent workgroups of a launch
(srcdsp_freqest_geometry).

The C ABI gives a bank call one n for all its rows, so "a row with n <= L among
long rows" cannot be asked of it; a bank call with n <= L follows a long one on
the same handle instead (test_bank_after_a_longer_call_and_below_L)."""
import numpy as np
import pytest

import freqest_model as M

pytestmark = pytest.mark.gpu

NBIG = 1 << 24


@pytest.fixture(scope="module")
def noise(S):
    """2^24 samples of +-32767 noise, on the host and on the device."""
    import torch
    x = np.random.default_rng(424242).integers(-32767, 32768, size=(NBIG, 2), dtype=np.int16)
    return x, torch.from_numpy(x).cuda()


@pytest.fixture(scope="module")
def geo(S):
    return S.FreqEstimator(1).geometry()


def check(got, x, L, what=None):
    f, sums, exact = got
    wf, wsums, wexact = M.estimate(x, L)
    assert (int(sums[0]), int(sums[1])) == wsums, what
    assert M.bits(f) == M.bits(wf), what
    assert bool(exact) == wexact, what


def test_geometry(S, geo):
    T, W, G = geo
    assert W == 4 and T % (64 * W) == 0 and G >= 1


@pytest.mark.parametrize("L", [1, 2, 3, 4, 7, 8, 32, 33, 1000, "T", "T+1"])
def test_single_row_lengths(S, noise, geo, L):
    x, xd = noise
    T, W, G = geo
    L = {"T": T, "T+1": T + 1}.get(L, L)
    e = S.FreqEstimator(L)
    for n in sorted({0, 1, L, L + 1, L + 2, 63, 64, 65, T - 1, T, T + 1, T + L, 2 * T + 3, 3 * T + W - 1}):
        check(e.run(xd[:n]), x[:n], L, (L, n))


@pytest.mark.parametrize("L", [1, 33])
def test_one_full_pass_of_all_workgroups_and_one_pair_more(S, noise, geo, L):
    """n - L = G T gives every persistent workgroup one tile; one pair more
    gives a workgroup a second tile."""
    x, xd = noise
    T, W, G = geo
    assert G * T + L + 1 <= NBIG
    e = S.FreqEstimator(L)
    for n in (G * T + L, G * T + L + 1):
        check(e.run(xd[:n]), x[:n], L, (L, n))


@pytest.mark.parametrize("L", [1, 3])
def test_every_start_alignment(S, noise, geo, L):
    """The same row at every start offset 0 .. W-1 samples into an allocation:
    4-byte aligned, not 16-byte aligned."""
    import torch
    x, xd = noise
    T, W, G = geo
    n = 2 * T + 3
    e = S.FreqEstimator(L)
    want = M.estimate(x[:n], L)
    for o in range(W):
        buf = torch.full((n + W, 2), 32767, dtype=torch.int16, device="cuda")
        buf[o:o + n] = xd[:n]
        row = buf[o:o + n]
        assert row.data_ptr() % 16 == (4 * o) % 16
        f, sums, exact = e.run(row)
        assert sums == want[1] and M.bits(f) == M.bits(want[0]) and exact == want[2], o


def test_large_run_every_workgroup_loops(S, noise, geo):
    x, xd = noise
    T, W, G = geo
    assert NBIG // T >= 2 * G
    check(S.FreqEstimator(3).run(xd), x, 3)


def test_scratch_reuse_large_then_short_then_below_L(S, noise):
    x, xd = noise
    e = S.FreqEstimator(5)
    for n in (1 << 22, 100, 5, 4, 1 << 14, 6):
        check(e.run(xd[:n]), x[:n], 5, n)


def test_full_scale_at_the_exactness_bound(S):
    """All samples (32767, 32767): every termI is 2 * 32767^2.  At 2^22 pairs
    the bound holds; 4097 pairs more and it does not, the sums staying exact."""
    import torch
    L, T2 = 1, 2 * 32767 ** 2
    xd = torch.full(((1 << 22) + 4097 + L, 2), 32767, dtype=torch.int16, device="cuda")
    e = S.FreqEstimator(L)
    f, sums, exact = e.run(xd[:(1 << 22) + L])
    assert sums == ((1 << 22) * T2, 0) and exact is True and M.bits(f) == 0
    f, sums, exact = e.run(xd)
    assert sums == (((1 << 22) + 4097) * T2, 0) and exact is False and M.bits(f) == 0


@pytest.mark.parametrize("L", [1, 4])
def test_wrap_corner(S, noise, geo, L):
    """Runs of (-32768, -32768): termI = 2^31 wraps to -2^31."""
    import torch
    x, _ = noise
    T, W, G = geo
    n = 2 * T + 7
    y = x[:n].copy()
    y[10:10 + 3 * L] = -32768
    y[T - 2:T + L + 2] = -32768
    y[n - L - 1:] = -32768
    ti, _ = M.terms(y, L)
    assert int((ti == -(1 << 31)).sum()) > 4
    check(S.FreqEstimator(L).run(torch.from_numpy(y).cuda()), y, L)
    z = np.full((n, 2), -32768, np.int16)
    f, sums, exact = S.FreqEstimator(L).run(torch.from_numpy(z).cuda())
    assert sums == (-(n - L) << 31, 0) and exact and M.bits(f) == M.bits(np.float32(np.pi / L))


@pytest.mark.parametrize("n", [17, 4097])
@pytest.mark.parametrize("C_", [1, 3, 64, 65])
def test_bank(S, noise, C_, n):
    """Rows at odd offsets inside rows of full-scale samples, rows laid back to
    back in one buffer, and overlapping rows of one buffer: each row equals the
    single-row call and the model.  A pair or a load that crossed a row seam
    would meet a full-scale neighbour and change the sum."""
    import torch
    x, xd = noise
    rng = np.random.default_rng(100 * C_ + n)
    for L in (1, 4):
        e, one = S.FreqEstimator(L), S.FreqEstimator(L)
        # (a) [C, m, 2]: row c at an odd offset, full-scale samples around it
        m = n + 8
        offs = [1 + 2 * (c % 4) for c in range(C_)]
        buf = (32767 * (2 * rng.integers(0, 2, size=(C_, m, 2)) - 1)).astype(np.int16)
        for c in range(C_):
            buf[c, offs[c]:offs[c] + n] = x[c * n:(c + 1) * n]
        bd = torch.from_numpy(buf).cuda()
        f, sums, exact = e.run_batched(bd, offsets=offs, n=n)
        for c in range(C_):
            row = buf[c, offs[c]:offs[c] + n]
            check((f[c], sums[c], exact[c]), row, L, ("a", L, c))
            check(one.run(bd[c, offs[c]:offs[c] + n]), row, L, ("a1", L, c))
        # (b) one buffer, rows back to back from sample 1 on: noise rows between full-scale rows
        flat = np.empty((1 + C_ * n + 1, 2), np.int16)
        flat[:] = 32767
        for c in range(0, C_, 2):
            flat[1 + c * n:1 + (c + 1) * n] = x[c * n:(c + 1) * n]
        offs = [1 + c * n for c in range(C_)]
        f, sums, exact = e.run_batched(torch.from_numpy(flat).cuda(), offsets=offs, n=n, shared=True)
        for c in range(C_):
            check((f[c], sums[c], exact[c]), flat[offs[c]:offs[c] + n], L, ("b", L, c))
        # (c) in_stride = 0: overlapping rows of one buffer, the last ending at its end
        offs = [int(o) for o in rng.integers(0, 64, C_)]
        offs[-1] = 64
        f, sums, exact = e.run_batched(xd[:n + 64], offsets=offs, n=n, shared=True)
        for c in range(C_):
            check((f[c], sums[c], exact[c]), x[offs[c]:offs[c] + n], L, ("c", L, c))
        # no offsets: rows of a [C, n, 2] tensor
        f, sums, exact = e.run_batched(xd[:C_ * n].reshape(C_, n, 2))
        for c in range(C_):
            check((f[c], sums[c], exact[c]), x[c * n:(c + 1) * n], L, ("d", L, c))


def test_bank_rows_longer_than_a_tile_share_the_workgroups(S, noise, geo):
    """3 rows of several tiles: every row gets workgroups of its own and the
    finish step sums each row's slabs."""
    x, xd = noise
    T, W, G = geo
    n = 5 * T + 3
    e = S.FreqEstimator(2)
    f, sums, exact = e.run_batched(xd[:3 * (n + 1)].reshape(3, n + 1, 2), offsets=[1, 0, 1], n=n)
    for c, o in enumerate((1, 0, 1)):
        lo = c * (n + 1) + o
        check((f[c], sums[c], exact[c]), x[lo:lo + n], 2, c)


def test_bank_after_a_longer_call_and_below_L(S, noise):
    x, xd = noise
    L = 4
    e = S.FreqEstimator(L)
    e.run_batched(xd[:64 * 8192].reshape(64, 8192, 2))
    f, sums, exact = e.run_batched(xd[:3 * 40].reshape(3, 40, 2))
    for c in range(3):
        check((f[c], sums[c], exact[c]), x[c * 40:(c + 1) * 40], L, c)
    for n in (L, 1, 0):  # n <= L: zeros, +0.0f, exact
        f, sums, exact = e.run_batched(xd[:3 * 40].reshape(3, 40, 2), n=n)
        assert [M.bits(v) for v in f] == [0] * 3 and not sums.any() and exact.all()


def test_bank_scratch_grows_and_is_reused(S, noise):
    """The result rows and the row offsets live on the handle and only grow: one
    handle through calls of 2, 5 and 2 rows with offsets (kept, regrown, reused
    at the larger capacity), each row against the single-row call of a second
    handle (a handle has no signal state to clone) and the model."""
    x, xd = noise
    L, n = 1, 1024
    e, one = S.FreqEstimator(L), S.FreqEstimator(L)
    for call, ch in enumerate((2, 5, 2)):
        base = call * 5 * (n + 8)
        rows = xd[base:base + ch * (n + 8)].reshape(ch, n + 8, 2)
        offs = [1 + (c + call) % 7 for c in range(ch)]
        f, sums, exact = e.run_batched(rows, offsets=offs, n=n)
        for c in range(ch):
            lo = base + c * (n + 8) + offs[c]
            f1, s1, e1 = one.run(xd[lo:lo + n])
            assert (M.bits(f[c]), tuple(int(v) for v in sums[c]), bool(exact[c])) == (M.bits(f1), s1, e1), (call, c)
            check((f[c], sums[c], exact[c]), x[lo:lo + n], L, (call, c))


def test_run_host_equals_run(S, noise, geo):
    x, xd = noise
    T, W, G = geo
    for L, n in ((1, 3 * T + 5), (33, 100), (2, 2)):
        e = S.FreqEstimator(L)
        a, b = e.run(xd[:n]), e.run(x[:n])
        assert M.bits(a[0]) == M.bits(b[0]) and a[1:] == b[1:]
        check(b, x[:n], L)
    assert M.bits(S.estimate_freq(x[:1000], 2)) == M.bits(M.estimate(x[:1000], 2)[0])
