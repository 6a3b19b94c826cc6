"""The carrier combiner on device rows (srcdsp_combine_step) against the numpy
model, bit for bit: rows on both sides of the kernel's unroll by four, sample
counts on both sides of a lane's four samples and of a tile of 1024, rows off
16 bytes (the scalar path), one row shared, in place on row 0, both clamps, a
guard sample past the output."""
import ctypes as C

import numpy as np
import pytest

from combine_model import combine as model
from test_combine_capi import carriers

pytestmark = pytest.mark.gpu
ROWS, NS, SHIFTS = (1, 2, 3, 5, 64, 65), (1, 7, 8, 4096 * 3 + 5), (0, 2, 15)
GUARD = 77


def run(S, x, n, shift, base=0, in_place=False):
    """srcdsp_combine_step over the rows of x [rows, stride, 2], held in a
    device buffer `base` samples past a 16-byte boundary.  The output has a
    guard sample; in place it is row 0, and every other sample is unchanged."""
    import torch
    from srcdsp_amd import _capi as A
    rows, stride = x.shape[0], x.shape[1]
    buf = torch.zeros((rows * stride + base, 2), dtype=torch.int16, device="cuda")
    buf[base:] = torch.from_numpy(x.reshape(-1, 2)).cuda()
    src = buf[base:]
    assert src.data_ptr() % 16 == (4 * base) % 16
    out = src if in_place else torch.full((n + 1, 2), GUARD, dtype=torch.int16, device="cuda")
    A.call("srcdsp_combine_step", C.c_void_p(src.data_ptr()), stride, rows, C.c_void_p(out.data_ptr()), n, shift,
           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    y = out.cpu().numpy()
    if in_place:
        assert np.array_equal(y[n:], x.reshape(-1, 2)[n:])
        return y[:n]
    assert (y[n] == GUARD).all()
    return y[:n]


@pytest.mark.parametrize("rows", ROWS)
def test_aligned_rows(S, rows):
    for n in NS:
        stride = (n + 3) & ~3
        x = carriers(rows, n, 100 * rows + n % 97, stride=stride)
        for shift in SHIFTS:
            assert np.array_equal(run(S, x, n, shift), model(x[:, :n], shift)), (n, shift)


@pytest.mark.parametrize("rows", ROWS)
def test_rows_off_16_bytes_take_the_scalar_path(S, rows):
    """A stride that is no multiple of 4 samples, and a row base off 16 bytes."""
    for n in NS:
        x = carriers(rows, n, 200 * rows + n % 97, stride=n + 1 + (n % 4 == 3))
        assert x.shape[1] % 4 != 0
        if rows > 1:
            assert np.array_equal(run(S, x, n, 2), model(x[:, :n], 2)), n
        y = carriers(rows, n, 300 * rows + n % 97, stride=(n + 3) & ~3)
        assert np.array_equal(run(S, y, n, 0, base=1), model(y[:, :n], 0)), n


@pytest.mark.parametrize("rows", ROWS)
def test_in_place_on_row_0(S, rows):
    for n in NS:
        x = carriers(rows, n, 400 * rows + n % 97, stride=(n + 3) & ~3)
        assert np.array_equal(run(S, x, n, 2, in_place=True), model(x[:, :n], 2)), n
        assert np.array_equal(run(S, x, n, 0, base=3, in_place=True), model(x[:, :n], 0)), n


@pytest.mark.parametrize("rows", (1, 3, 8, 9))
def test_few_long_rows(S, rows):
    """2^22 samples and more: up to 8 rows take the kernel with one row in
    flight, 9 the other; one short of 2^22 takes the other too."""
    for n in ((1 << 22) - 1, (1 << 22) + 5):
        x = carriers(rows, n, 600 + rows, stride=(n + 3) & ~3)
        assert np.array_equal(run(S, x, n, 1), model(x[:, :n], 1)), n
    if rows == 3:
        assert np.array_equal(run(S, x, n, 0, base=1), model(x[:, :n], 0))                 # the scalar path
        assert np.array_equal(run(S, x, n, 2, in_place=True), model(x[:, :n], 2))          # in place


def test_one_row_shared(S):
    """in_stride == 0: the same row `rows` times, also in place."""
    import torch
    from srcdsp_amd import _capi as A
    for n in NS:
        row = carriers(1, n, 500 + n % 97)
        for rows in (1, 5, 65):
            want = model(np.repeat(row, rows, 0), 2)
            src = torch.from_numpy(row[0]).cuda()
            out = torch.full((n + 1, 2), GUARD, dtype=torch.int16, device="cuda")
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            A.call("srcdsp_combine_step", C.c_void_p(src.data_ptr()), 0, rows, C.c_void_p(out.data_ptr()), n, 2, st)
            y = out.cpu().numpy()
            assert np.array_equal(y[:n], want) and (y[n] == GUARD).all(), (n, rows)
            A.call("srcdsp_combine_step", C.c_void_p(src.data_ptr()), 0, rows, C.c_void_p(src.data_ptr()), n, 2, st)
            assert np.array_equal(src.cpu().numpy(), want), (n, rows)


def test_saturation_at_both_ends(S):
    x = carriers(65, 4096 * 3 + 5, 6, stride=4096 * 3 + 8)
    y = run(S, x, 4096 * 3 + 5, 0)
    assert y[0].tolist() == [-32768, 32767] and y[1].tolist() == [32767, -32768]
    assert y[2].tolist() == [-32768, 32767] and y[3].tolist() == [-32768, 32767]
    assert np.array_equal(y, model(x[:, :4096 * 3 + 5], 0))
    assert (y == 32767).sum() > 1000 and (y == -32768).sum() > 1000  # 65 random rows clamp often
    z = run(S, x, 4096 * 3 + 5, 15)
    assert z[0].tolist() == [-65, 64] and np.abs(z[4:]).max() < 32767


def test_python_face_on_device_tensors(S):
    import torch
    x = carriers(5, 1000, 7, stride=1004)
    wide = torch.from_numpy(x).cuda()
    want = model(x[:, :1000], 1)
    assert np.array_equal(S.combine(wide[:, :1000], shift=1).cpu().numpy(), want)        # a view of a wider buffer
    assert np.array_equal(S.combine([wide[c, :1000] for c in range(5)], shift=1).cpu().numpy(), want)
    assert np.array_equal(S.combine(wide[0, :1000]).cpu().numpy(), x[0, :1000])          # one row, shift 0
    out = wide[0, :1000]
    assert S.combine(wide[:, :1000], out, 1) is out                                      # in place on row 0
    assert np.array_equal(wide[0, :1000].cpu().numpy(), want)
    assert np.array_equal(wide[1:].cpu().numpy(), x[1:]) and np.array_equal(wide[0, 1000:].cpu().numpy(), x[0, 1000:])
    with pytest.raises(ValueError):
        S.combine([wide[0, :1000], wide[2, :1000], wide[3, :1000]])                      # not one spacing
    with pytest.raises(S.SrcdspError):
        S.combine(wide[:, :1000], shift=16)
    half = torch.zeros((2, 8, 2), dtype=torch.float16, device="cuda")                    # 2 bytes, but no int16
    for bad in (lambda: S.combine(half), lambda: S.combine([half[0], half[1]]),
                lambda: S.combine(wide[:, :8], half[0]),
                lambda: S.combine(wide[:, :8], torch.zeros((16, 2), dtype=torch.int16, device="cuda")[::2])):
        with pytest.raises(ValueError):
            bad()


def test_offsets_past_2_to_the_31(S):
    """Offsets are 64-bit: a second row 2^31 + 4 samples behind the first, and
    one row of 2^31 + 5 samples combined in place (the last tile starts past
    2^31).  One buffer of 8.6 GB serves both; only the compared parts are
    brought back."""
    import torch
    from srcdsp_amd import _capi as A
    stride, n_small = (1 << 31) + 4, 1029
    buf = torch.empty((stride + n_small, 2), dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = carriers(2, n_small, 8)
    buf[:n_small] = torch.from_numpy(x[0]).cuda()
    buf[stride:] = torch.from_numpy(x[1]).cuda()
    out = torch.full((n_small + 1, 2), GUARD, dtype=torch.int16, device="cuda")
    A.call("srcdsp_combine_step", C.c_void_p(buf.data_ptr()), stride, 2, C.c_void_p(out.data_ptr()), n_small, 0, st)
    y = out.cpu().numpy()
    assert np.array_equal(y[:n_small], model(x, 0)) and (y[n_small] == GUARD).all()
    n = (1 << 31) + 5
    buf.fill_(3)
    spots = {0: (-32768, 32767), 1023: (7, -9), (1 << 31) - 1: (101, -101), 1 << 31: (-5, 5), n - 1: (32767, -32768)}
    for i, v in spots.items():
        buf[i] = torch.tensor(v, dtype=torch.int16)
    A.call("srcdsp_combine_step", C.c_void_p(buf.data_ptr()), 0, 1, C.c_void_p(buf.data_ptr()), n, 1, st)
    for i, v in spots.items():
        assert buf[i].tolist() == [v[0] >> 1, v[1] >> 1], i
        buf[i] = 1
    assert bool((buf[:n] == 1).all()) and bool((buf[n:] == 3).all())
