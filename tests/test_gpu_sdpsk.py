"""The SDPSK demodulator on the GPU (srcdsp_sdpsk_step, _step_batched) against
the numpy model: soft bits, bits, carries and states bit for bit, for n below
D, around the workgroup tile and across tiles, each output alone and both,
guard bytes, the extreme products at a tile's edges, streams in chunks and on
two streams, inputs at every sample offset from a 16-byte boundary, banks
against the single calls, and refusals that change nothing."""
import copy
import ctypes as C

import numpy as np
import pytest

from sdpsk_model import SdpskModel

pytestmark = pytest.mark.gpu

GUARD = 8
EXTREME = (((-32768, -32768), (-32768, 32767)), ((-32768, -32768), (32767, -32768)))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def samples(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, 2)).astype(np.int16)


@pytest.fixture(scope="module")
def T(S):
    t, d, w = S.sdpsk_geometry()
    assert t in (1024, 2048, 4096) and d == 64
    assert w == 0  # not persistent: no tile loop to size a call for
    return t


def raw_step(d, xd, n, soft=True, bits=True, stream=None, lo_soft=0, lo_bits=0):
    """srcdsp_sdpsk_step into guarded buffers that start lo_* bytes past a
    256-byte boundary; the outputs on the host (None for one not asked for)."""
    import torch
    from srcdsp_amd import _capi as A
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        s = torch.full((lo_soft + n + GUARD,), 77, dtype=torch.int8, device="cuda")
        b = torch.full((lo_bits + n + GUARD,), 77, dtype=torch.uint8, device="cuda")
    A.call("srcdsp_sdpsk_step", d._h, C.c_void_p(xd.data_ptr()), n, C.c_void_p(s.data_ptr() + lo_soft) if soft else None,
           C.c_void_p(b.data_ptr() + lo_bits) if bits else None, C.c_void_p(st.cuda_stream))
    return s, b


def check(s, b, n, ms, mb, soft=True, bits=True, lo_soft=0, lo_bits=0, what=None):
    s, b = s.cpu().numpy(), b.cpu().numpy()
    for got, lo, want, on in ((s, lo_soft, ms, soft), (b, lo_bits, mb, bits)):
        assert (got[:lo] == 77).all() and (got[lo + n:] == 77).all(), what  # the guard bytes
        if on:
            assert np.array_equal(got[lo:lo + n], want), what
        else:
            assert (got == 77).all(), what


def same_state(d, m, what=None):
    D, shift, carry = d.state()
    assert (D, shift) == (m.D, m.shift) and np.array_equal(carry, m.carry), what


def with_extremes(x, D, T):
    """The largest product at a tile's first sample, the smallest at a tile's last."""
    n = len(x)
    for (a, b), i in zip(EXTREME, (T, 2 * T - 1)):
        if i < n:
            x[i], x[i - D] = a, b
    return x


@pytest.mark.parametrize("D", [1, 2, 4, 63, 64])
def test_step_equals_the_model(S, T, D):
    """One handle per D streams through every length, shift and output choice:
    the carry of each call is the next one's."""
    d, m = S.DemodulatorSdpsk(D, 0), SdpskModel(D, 0)
    k = 0
    for shift in (0, 17, 31):
        d.setShift(shift)
        m.shift = shift
        for n in (0, 1, D - 1, D, D + 1, T - 1, T, T + 1, 2 * T + 3):
            for soft, bits in ((True, False), (False, True), (True, True)):
                k += 1
                x = with_extremes(samples(n, 1000 * D + k), D, T)
                s, b = raw_step(d, dev(x) if n else dev(np.zeros((1, 2), np.int16)), n, soft, bits)
                ms, mb = m.step(x)
                check(s, b, n, ms, mb, soft, bits, what=(shift, n, soft, bits))
                same_state(d, m, (shift, n))
                if n == 2 * T + 3 and shift == 0 and soft:
                    assert ms[T] == 127 and ms[2 * T - 1] == -128 and mb[T] == 1 and mb[2 * T - 1] == 0


def test_extremes_with_the_predecessor_in_the_carry(S, T):
    """The extreme pairs across a call: b is the carry's last sample, a the call's first."""
    for (a, b), soft, bit in zip(EXTREME, (127, -128), (1, 0)):
        d = S.DemodulatorSdpsk(1, 24)
        d.step(dev(np.array([b], np.int16)))
        s, bt = d.step(dev(np.array([a], np.int16)))
        assert s.cpu().numpy().tolist() == [soft] and bt.cpu().numpy().tolist() == [bit]


@pytest.mark.parametrize("D", [1, 5, 64])
def test_stream_in_chunks(S, T, D):
    """3T + 5 samples in chunks (T + 1, D - 1, 1, rest): the carry crosses calls
    and tiles, a call shorter than D included."""
    x = samples(3 * T + 5, 40 + D)
    whole_s, whole_b = SdpskModel(D, 13).step(x)
    d, m = S.DemodulatorSdpsk(D, 13), SdpskModel(D, 13)
    at, got_s, got_b = 0, [], []
    for n in (T + 1, D - 1, 1, 3 * T + 5 - (T + 1) - (D - 1) - 1):
        if n:
            s, b = d.step(dev(x[at:at + n]))
            got_s.append(s.cpu().numpy())
            got_b.append(b.cpu().numpy())
        m.step(x[at:at + n])
        at += n
        same_state(d, m, n)
    assert at == len(x)
    assert np.array_equal(np.concatenate(got_s), whole_s) and np.array_equal(np.concatenate(got_b), whole_b)


def test_two_chunks_on_two_streams_are_ordered(S, T):
    """The second chunk, on another stream, reads the carry the first one's last
    tile writes: no synchronisation in between but the handle's own."""
    import torch
    D, n0, n1 = 64, 64 * T + 7, 2 * T + 1
    x = samples(n0 + n1, 50)
    xd = dev(x)
    m = SdpskModel(D, 16)
    d = S.DemodulatorSdpsk(D, 16)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = raw_step(d, xd[:n0], n0, stream=s1)
    b = raw_step(d, xd[n0:], n1, stream=s2)
    torch.cuda.synchronize()
    check(*a, n0, *m.step(x[:n0]))
    check(*b, n1, *m.step(x[n0:]))
    same_state(d, m)


@pytest.mark.parametrize("lo", [1, 2, 3])
def test_input_off_a_16_byte_boundary(S, T, lo):
    """An input base at +1, +2, +3 samples from a 16-byte boundary, whole and
    partial tiles; then outputs off a 4-byte boundary as well (byte stores)."""
    D = 3
    x = samples(2 * T + 16, 60 + lo)
    xd = dev(x)
    assert xd.data_ptr() % 16 == 0
    d, m = S.DemodulatorSdpsk(D, 14), SdpskModel(D, 14)
    for n in (1, 2, 5, T - lo, T, T + 1, 2 * T + 3):
        for lo_s, lo_b in ((0, 0), (lo, 4 - lo)):
            s, b = raw_step(d, xd[lo:lo + n], n, lo_soft=lo_s, lo_bits=lo_b)
            ms, mb = m.step(x[lo:lo + n])
            check(s, b, n, ms, mb, lo_soft=lo_s, lo_bits=lo_b, what=(n, lo_s, lo_b))
            same_state(d, m, n)


def primed(S, D, shift, seed):
    """A demodulator whose carry the device holds, and the model of the same."""
    d, m = S.DemodulatorSdpsk(D, shift), SdpskModel(D, shift)
    x = samples(D + 3, seed)
    d.step(dev(x))
    m.step(x)
    return d, m


@pytest.mark.parametrize("D", [1, 4, 64])
def test_bank_equals_the_single_calls(S, T, D):
    """5 rows with odd in_offsets, output strides wider than n, a carry of its
    own per row: rows one buffer each, then in_stride == 0 with offsets into one
    row.  Every handle ends as its single call leaves it."""
    import torch
    from srcdsp_amd import _capi as A
    rows, shift = 5, 15
    pairs = [primed(S, D, shift, 70 + r) for r in range(rows)]
    for n, shared in ((T + 9, False), (2 * T + 3, True), (D - 1, False), (7, True)):
        if n == 0:
            continue
        offs = [3, T + 1, 5, 2 * T + 2, 9] if shared else [1, 3, 0, 7, 13]
        m_in = n + max(offs)
        x = samples(m_in, n) if shared else samples(rows * m_in, n).reshape(rows, m_in, 2)
        xd = dev(x)
        singles = [copy.copy(d) for d, _ in pairs]
        ss, bs = n + 5, n + 8  # strides wider than n, the soft rows off 4-byte boundaries
        soft = torch.full((rows, ss), 77, dtype=torch.int8, device="cuda")
        bits = torch.full((rows, bs), 77, dtype=torch.uint8, device="cuda")
        A.call("srcdsp_sdpsk_step_batched", (C.c_void_p * rows)(*[d._h.value for d, _ in pairs]), rows,
               C.c_void_p(xd.data_ptr()), 0 if shared else m_in, (C.c_size_t * rows)(*offs), n,
               C.c_void_p(soft.data_ptr()), ss, C.c_void_p(bits.data_ptr()), bs,
               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        s, b = soft.cpu().numpy(), bits.cpu().numpy()
        assert (s[:, n:] == 77).all() and (b[:, n:] == 77).all()
        for r, (d, m) in enumerate(pairs):
            row = x[offs[r]:offs[r] + n] if shared else x[r, offs[r]:offs[r] + n]
            ms, mb = m.step(row)
            assert np.array_equal(s[r, :n], ms) and np.array_equal(b[r, :n], mb), (n, r)
            one_s, one_b = singles[r].step(dev(row))
            assert np.array_equal(one_s.cpu().numpy(), ms) and np.array_equal(one_b.cpu().numpy(), mb)
            same_state(d, m, (n, r))
            assert np.array_equal(singles[r].state()[2], d.state()[2])


def test_python_bank_face(S, T):
    """sdpsk_step_batched: all the hits of one stream, and a row per channel."""
    D = 2
    pairs = [primed(S, D, 12, 90 + r) for r in range(3)]
    x = samples(T + 40, 91)
    offs = [1, 18, 37]
    soft, bits = S.sdpsk_step_batched([d for d, _ in pairs], dev(x), offsets=offs, n=T + 3)
    assert soft.shape == (3, T + 3) and bits.shape == (3, T + 3)
    for r, (d, m) in enumerate(pairs):
        ms, mb = m.step(x[offs[r]:offs[r] + T + 3])
        assert np.array_equal(soft[r].cpu().numpy(), ms) and np.array_equal(bits[r].cpu().numpy(), mb)
        same_state(d, m, r)
    xr = samples(3 * 50, 92).reshape(3, 50, 2)
    soft, bits = S.sdpsk_step_batched([d for d, _ in pairs], dev(xr))
    for r, (d, m) in enumerate(pairs):
        ms, mb = m.step(xr[r])
        assert np.array_equal(soft[r].cpu().numpy(), ms) and np.array_equal(bits[r].cpu().numpy(), mb)
        same_state(d, m, r)
    # back-to-back banks led by the same handle, more than its ring of row tables has slots
    xd = dev(x)
    outs = [S.sdpsk_step_batched([d for d, _ in pairs], xd, offsets=[k, k + 6, k + 13], n=T) for k in range(7)]
    for k, (soft, bits) in enumerate(outs):
        for r, (d, m) in enumerate(pairs):
            lo = (k, k + 6, k + 13)[r]
            ms, mb = m.step(x[lo:lo + T])
            assert np.array_equal(soft[r].cpu().numpy(), ms) and np.array_equal(bits[r].cpu().numpy(), mb), (k, r)
    for r, (d, m) in enumerate(pairs):
        same_state(d, m, r)


def test_bank_of_more_rows_than_a_launch_takes(S, T):
    """65 535 + 3 rows: two launches (the grid's y limit) share one row table.
    Every row is 5 samples at its own offset into one buffer."""
    rows, n, D = 65535 + 3, 5, 2
    x = samples(64 + n, 93)
    offs = [(7 * c) % 64 for c in range(rows)]
    demods = [S.DemodulatorSdpsk(D, 16) for _ in range(rows)]
    soft, bits = S.sdpsk_step_batched(demods, dev(x), offsets=offs, n=n)
    soft, bits = soft.cpu().numpy(), bits.cpu().numpy()
    want = [SdpskModel(D, 16).step(x[o:o + n]) for o in range(64)]
    idx = np.array(offs)
    assert np.array_equal(soft, np.stack([w[0] for w in want])[idx])
    assert np.array_equal(bits, np.stack([w[1] for w in want])[idx])
    for c in (0, 1, 65534, 65535, 65536, rows - 1):  # on both sides of the split
        assert np.array_equal(demods[c].state()[2], x[offs[c] + n - D:offs[c] + n]), c


def test_refusals_change_nothing(S, T):
    from srcdsp_amd import _capi as A
    g, m = primed(S, 4, 10, 95)
    h, mh = primed(S, 5, 10, 96)
    k, mk = primed(S, 4, 11, 97)
    x = samples(64, 98)
    xd = dev(x)

    def refused(code, fn):
        with pytest.raises(S.SrcdspError) as e:
            fn()
        assert e.value.code == code

    refused(A.ERR_ARG, lambda: S.sdpsk_step_batched([g, g], xd))  # listed twice
    refused(A.ERR_ARG, lambda: S.sdpsk_step_batched([g, h], xd))  # D differs
    refused(A.ERR_ARG, lambda: S.sdpsk_step_batched([g, k], xd))  # the shift differs
    for d, mm in ((g, m), (h, mh), (k, mk)):
        same_state(d, mm)
        s, b = d.step(xd)
        ms, mb = mm.step(x)
        assert np.array_equal(s.cpu().numpy(), ms) and np.array_equal(b.cpu().numpy(), mb)


def test_host_step_after_device_steps_and_reset(S, T):
    """A numpy input runs on the host from the carry the device holds; reset and
    copy on a handle the device holds."""
    d, m = primed(S, 7, 9, 99)
    x = samples(T + 30, 100)
    for part in (x[:5], x[5:T], x[T:]):
        s, b = d.step(part)  # numpy in: srcdsp_sdpsk_step_host
        ms, mb = m.step(part)
        assert np.array_equal(s, ms) and np.array_equal(b, mb)
        s, b = d.step(dev(part))
        ms, mb = m.step(part)
        assert np.array_equal(s.cpu().numpy(), ms) and np.array_equal(b.cpu().numpy(), mb)
    c = copy.copy(d)
    d.reset()
    m2 = SdpskModel(7, 9)
    assert np.array_equal(d.step(dev(x[:100]))[0].cpu().numpy(), m2.step(x[:100])[0])
    same_state(c, m)
    assert np.array_equal(c.step(dev(x[:100]))[1].cpu().numpy(), m.step(x[:100])[1])
