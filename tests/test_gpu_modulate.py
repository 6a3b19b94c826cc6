"""The transmit chain from bits (srcdsp_modulate_step, _step_batched): the two
chain goldens recorded from the reference's mapper -> FilterUpsamplingFir ->
Mixer; the fused call against the sequence srcdsp_mapper_step ->
srcdsp_upmix_step on clones, outputs and all three handles' state bit for bit;
the counters say which path served a call; banks against the loop; refusals
change no handle.

TI = 2048 symbols is the interpolator tile.  The interpolator's history is
compared through a further (flushing) step of both chains."""
import copy
import ctypes as C

import numpy as np
import pytest

import mapper_model as M

pytestmark = pytest.mark.gpu

TI = 2048
MAN, ARR = M.load_golden()
BYTES = np.array(MAN["bit_bytes"], np.uint8)
UP_T = {0: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t"),
        1: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int16_t"),
        2: ("int16_t", "int16_t", "int32_t", "int32_t")}


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def random_bits(n, seed):
    return np.random.default_rng(seed).choice(BYTES, n)


def taps(L, ntaps):
    from srcdsp_amd.design import hamming_sinc, q14
    return q14(hamming_sinc(ntaps, 0.48 / L) * L)


class Chain:
    """The three operators of one channel."""

    def __init__(self, S, kind, c, L, f, state=0, variant=0, N=4096):
        self.S, self.kind = S, kind
        self.mapper = (S.SymbolMapperQpsk if kind == M.QPSK else S.SymbolMapperSdpsk)()
        self.mapper.setState(state)
        self.up = S.FilterUpsamplingFir(c, L, *UP_T[variant])
        self.mixer = S.Mixer(N)
        self.mixer.reset(f)

    def clone(self):
        c = copy.copy(self)
        c.mapper, c.up, c.mixer = copy.copy(self.mapper), copy.copy(self.up), copy.copy(self.mixer)
        return c

    def fused(self, bits_d, flush=False):
        return self.S.ModulatorChain(self.mapper, self.up, self.mixer).step(bits_d, None, flush)

    def sequence(self, bits_d, flush=False):
        sym = self.mapper.step(bits_d)
        return self.S.UpsamplerMixerChain(self.up, self.mixer).step(sym, None, flush)

    def state(self):
        return self.mapper.state(), self.mixer.state()[:2]

    def bits_for(self, n_sym):
        return n_sym * (2 if self.kind == M.QPSK else 1)


def same_state(a: Chain, b: Chain, seed=99):
    """Mapper state, mixer phase, and the interpolator's history as a further
    flushing step shows it (on clones, so a and b stay as they are)."""
    assert a.state() == b.state()
    a2, b2 = a.clone(), b.clone()
    bits = dev(random_bits(a.bits_for(40), seed))
    assert np.array_equal(a2.sequence(bits, True).cpu().numpy(), b2.sequence(bits, True).cpu().numpy())
    assert a2.state() == b2.state()


def stats_delta(S, fn):
    s0 = S.modulate_stats()
    r = fn()
    return r, tuple(b - a for a, b in zip(s0, S.modulate_stats()))


# ----------------------------------------------------------------- goldens
@pytest.mark.parametrize("chain", MAN["chains"], ids=[c["key"] for c in MAN["chains"]])
def test_chain_goldens(S, chain):
    k = chain["key"]
    ch = Chain(S, chain["kind"], ARR[k + "_taps"], chain["L"], chain["freq"], N=chain["N"])
    bits, pos, ys = ARR[k + "_bits"], 0, []
    for n, flush in zip(chain["calls"], chain["flush"]):
        bd = dev(bits[pos:pos + n])  # its own allocation: 16-byte aligned
        y, d = stats_delta(S, lambda: ch.fused(bd, flush))
        assert d == (1, 0, 0, 0)
        ys.append(y.cpu().numpy())
        pos += n
    assert np.array_equal(np.concatenate(ys), ARR[k + "_out"])


# ------------------------------------------------- fused against the sequence
# (4, 16): 2 pairs per phase, run-time; (4, 128): 16 pairs per phase, compiled in; (3, 15): run-time L
@pytest.mark.parametrize("L,ntaps", [(4, 16), (4, 128), (3, 15)])
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_fused_equals_the_sequence(S, kind, L, ntaps):
    c = taps(L, ntaps)
    base = Chain(S, kind, c, L, 0.1137, state=3)
    base.sequence(dev(random_bits(base.bits_for(100), 1)))  # a history, a phase, a state to start from
    for k, n_sym in enumerate((TI - 1, TI, TI + 1, 2 * TI + 5)):
        bd = dev(random_bits(base.bits_for(n_sym), 10 + k))
        for flush in (False, True):
            a, b = base.clone(), base.clone()
            y, d = stats_delta(S, lambda: a.fused(bd, flush))
            assert d == (1, 0, 0, 0), "the fused kernel serves these shapes"
            want = b.sequence(bd, flush)
            assert y.shape == want.shape and np.array_equal(y.cpu().numpy(), want.cpu().numpy()), (n_sym, flush)
            same_state(a, b)


@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_sequence_equals_model_and_oracle(S, O, kind):
    """The yardstick of the test above is itself the reference's three calls."""
    c = taps(4, 16)
    bits = random_bits((2 if kind == M.QPSK else 1) * (TI + 1), 3)
    ch = Chain(S, kind, c, 4, 0.1137, state=1)
    y = ch.fused(dev(bits), True).cpu().numpy()
    mixer = O["strict"].mixer(4096)
    mixer.reset(0.1137)
    want = mixer.step(O["strict"].up(0, 4, c).step(M.MapperModel(kind, 1).step(bits), True))
    assert np.array_equal(y, np.asarray(want).reshape(-1, 2))


@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_stream_in_two_chunks_equals_one_call(S, kind):
    c = taps(4, 128)
    one = Chain(S, kind, c, 4, -0.3021, state=2)
    two = one.clone()
    n0, n1 = one.bits_for(1000), one.bits_for(1049)
    bd = dev(random_bits(n0 + n1, 4))
    whole = one.fused(bd).cpu().numpy()
    (y0, y1), d = stats_delta(S, lambda: (two.fused(bd[:n0]), two.fused(bd[n0:])))
    # the second chunk's bits start at byte 2000 (QPSK, 16-byte aligned: the fused kernel again) or at byte
    # 1000 (SDPSK, not aligned: the chain path continues what the fused kernel left)
    assert d == ((2, 0, 0, 0) if kind == M.QPSK else (1, 1, 0, 0))
    assert np.array_equal(np.concatenate([y0.cpu().numpy(), y1.cpu().numpy()]), whole)
    same_state(one, two)


# ---------------------------------------------------------------- chain path
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_chain_path_serves_what_the_fused_kernel_does_not(S, kind):
    n_sym = TI + 7
    # int16 taps (variant 1)
    c16 = taps(4, 16).astype(np.int16)
    a = Chain(S, kind, c16, 4, 0.1137, state=1, variant=1)
    b = a.clone()
    bits = random_bits(a.bits_for(n_sym) + 16, 6)
    bd = dev(bits)
    for flush in (False, True):
        y, d = stats_delta(S, lambda: a.fused(bd[16:], flush))
        assert d == (0, 1, 0, 0)
        assert np.array_equal(y.cpu().numpy(), b.sequence(bd[16:], flush).cpu().numpy())
        same_state(a, b)
    # d_bits off by one byte: the same results as the aligned call
    f, g = Chain(S, kind, taps(4, 16), 4, 0.1137, state=1), Chain(S, kind, taps(4, 16), 4, 0.1137, state=1)
    n = f.bits_for(n_sym)
    aligned = dev(bits[1:1 + n])
    y, d = stats_delta(S, lambda: f.fused(bd[1:1 + n], True))
    assert d == (0, 1, 0, 0)
    want, d = stats_delta(S, lambda: g.fused(aligned, True))
    assert d == (1, 0, 0, 0)
    assert np.array_equal(y.cpu().numpy(), want.cpu().numpy())
    same_state(f, g)


# --------------------------------------------------------------------- banks
@pytest.mark.parametrize("shared", [True, False], ids=["shared_bits", "bits_per_row"])
@pytest.mark.parametrize("rows", [3, 65])
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_bank_equals_the_loop(S, kind, rows, shared):
    """65 rows cross kMaxBatch = 64; every row has its own start state,
    carrier and history."""
    import torch
    L, n_sym = 4, 300
    c = taps(L, 16)
    chains = [Chain(S, kind, c, L, 0.01 * (r + 1), state=r % 4) for r in range(rows)]
    n = chains[0].bits_for(n_sym)
    for r, ch in enumerate(chains):
        ch.sequence(dev(random_bits(ch.bits_for(8 + r % 5), r)))
    loop = [ch.clone() for ch in chains]
    stride = (n + 15) // 16 * 16
    bits = random_bits(rows * stride, 8).reshape(rows, stride)
    bd = dev(bits[0, :n]) if shared else dev(bits)[:, :n]
    for flush in (False, True):
        n_out = L * (n_sym + (chains[0].up.getLength() // L if flush else 0))
        out = torch.full((rows, n_out + 8, 2), 77, dtype=torch.int16, device="cuda")
        _, d = stats_delta(S, lambda: bank(S, chains, bd, 0 if shared else stride, out, n, flush))
        assert d == (0, 0, 1, 0), "one launch per 64 rows serves this shape"
        y = out.cpu().numpy()
        assert (y[:, n_out:] == 77).all()
        for r in range(rows):
            row = bd if shared else dev(bits[r, :n])
            assert np.array_equal(y[r, :n_out], loop[r].sequence(row, flush).cpu().numpy()), (flush, r)
        for a, b in zip(chains, loop):
            assert a.state() == b.state()
    for r in (0, rows - 1):
        same_state(chains[r], loop[r])


def bank(S, chains, bits_d, bits_stride, out, n_bits, flush):
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles, _ptr, _stream
    A.call("srcdsp_modulate_step_batched", _handles([c.mapper for c in chains]), _handles([c.up for c in chains]),
           _handles([c.mixer for c in chains]), len(chains), C.c_void_p(bits_d.data_ptr()), bits_stride, _ptr(out),
           out.shape[1], n_bits, int(flush), _stream(out))


def test_bank_loop_path_and_python_face(S):
    """Row strides that are no multiple of 16 bytes: the per-channel loop,
    through the Python face, equal to the single calls."""
    import torch
    rows, L, n = 3, 4, 301
    c = taps(L, 16)
    chains = [Chain(S, M.SDPSK, c, L, 0.02 * (r + 1), state=r) for r in range(rows)]
    loop = [ch.clone() for ch in chains]
    bits = random_bits(rows * n, 9).reshape(rows, n)
    out = torch.zeros((rows, L * n, 2), dtype=torch.int16, device="cuda")
    _, d = stats_delta(S, lambda: S.modulate_step_batched([c.mapper for c in chains], [c.up for c in chains],
                                                          [c.mixer for c in chains], dev(bits), out))
    assert d == (0, 0, 0, 1)
    for r in range(rows):
        assert np.array_equal(out[r].cpu().numpy(), loop[r].sequence(dev(bits[r])).cpu().numpy())
        same_state(chains[r], loop[r])


# ----------------------------------------------------------------- refusals
def test_refusals_leave_every_handle_unchanged(S):
    import torch
    from srcdsp_amd import _capi as A
    c = taps(4, 16)
    chains = [Chain(S, M.QPSK, c, 4, 0.1 * (r + 1), state=r + 1) for r in range(2)]
    for ch in chains:
        ch.sequence(dev(random_bits(64, 2)))
    keep = [ch.clone() for ch in chains]
    a, b = chains
    bd = dev(random_bits(64, 3))
    out = torch.zeros((2, 4 * 32 + 64, 2), dtype=torch.int16, device="cuda")
    st0 = S.modulate_stats()

    def refused(code, fn):
        with pytest.raises(S.SrcdspError) as e:
            fn()
        assert e.value.code == code

    single = S.ModulatorChain(a.mapper, a.up, a.mixer)
    refused(A.ERR_SIZE, lambda: single.step(bd, out[0, :4 * 32 + 1]))          # a wrong n_out
    refused(A.ERR_SIZE, lambda: single.step(bd, out[0, :4 * 32], True))        # no room for the flush
    refused(A.ERR_SIZE, lambda: single.step(bd[:63], out[0, :4 * 31]))         # an odd QPSK bit count
    real = S.FilterUpsamplingFir(c, 4, *UP_T[2])
    refused(A.ERR_UNSUPPORTED, lambda: S.ModulatorChain(a.mapper, real, a.mixer).step(bd, out[0, :4 * 32]))
    maps, ups, mixers = [a.mapper, b.mapper], [a.up, b.up], [a.mixer, b.mixer]
    go = lambda m, u, x, bits=bd, o=out: S.modulate_step_batched(m, u, x, bits, o)  # noqa: E731
    refused(A.ERR_ARG, lambda: go([a.mapper, a.mapper], ups, mixers))           # listed twice
    refused(A.ERR_ARG, lambda: go(maps, [a.up, a.up], mixers))
    refused(A.ERR_ARG, lambda: go(maps, ups, [b.mixer, b.mixer]))
    refused(A.ERR_ARG, lambda: go([a.mapper, S.SymbolMapperSdpsk()], ups, mixers))                     # kinds differ
    refused(A.ERR_ARG, lambda: go(maps, [a.up, S.FilterUpsamplingFir(taps(4, 20), 4, *UP_T[0])], mixers))  # taps differ
    refused(A.ERR_ARG, lambda: go(maps, [a.up, S.FilterUpsamplingFir(taps(2, 16), 2, *UP_T[0])], mixers))  # L differs
    refused(A.ERR_ARG, lambda: go(maps, ups, [a.mixer, S.Mixer(1024)]))                               # N differs
    short = torch.zeros((2, 4 * 32 - 1, 2), dtype=torch.int16, device="cuda")
    refused(A.ERR_SIZE, lambda: go(maps, ups, mixers, o=short))                                        # out_stride short
    refused(A.ERR_SIZE, lambda: go(maps, ups, mixers, bits=bd[:63]))                                   # odd QPSK bits
    assert S.modulate_stats() == st0
    for ch, k in zip(chains, keep):
        same_state(ch, k)
