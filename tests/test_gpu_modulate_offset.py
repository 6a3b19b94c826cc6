"""The offset-QPSK transmit chain from bits (srcdsp_modulate_offset_step,
_step_batched): the fused call against the four calls srcdsp_mapper_step ->
srcdsp_up_step -> srcdsp_stagger_step -> srcdsp_mixer_step on clones and
against the mapper model, the oracle's interpolator and mixer and the stagger
model, outputs and all four handles' state bit for bit; the goldens recorded
from the reference build; streams in chunks; the counters say which path served
a call; banks against the loop; refusals change no handle.

TI = 2048 symbols is the interpolator tile, a wave covers 512.  The
interpolator's history is compared through a further (flushing) step of both
chains."""
import copy
import ctypes as C

import numpy as np
import pytest

import mapper_model as M
import stagger_model as G

pytestmark = pytest.mark.gpu

TI = 2048
BYTES = np.array([0, 1, 2, 128, 255], np.uint8)
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
    """The four operators of one channel."""

    def __init__(self, S, kind, c, L, D, f, state=0, variant=0, N=4096):
        self.S, self.kind = S, kind
        self.mapper = (S.SymbolMapperQpsk if kind == M.QPSK else S.SymbolMapperSdpsk)()
        self.mapper.setState(state)
        self.up = S.FilterUpsamplingFir(c, L, *UP_T[variant])
        self.stagger = S.QStagger(D)
        self.mixer = S.Mixer(N)
        self.mixer.reset(f)

    def clone(self):
        c = copy.copy(self)
        c.mapper, c.up = copy.copy(self.mapper), copy.copy(self.up)
        c.stagger, c.mixer = copy.copy(self.stagger), copy.copy(self.mixer)
        return c

    def handles(self):
        return self.mapper, self.up, self.stagger, self.mixer

    def fused(self, bits_d, flush=False, iterator=False):
        return self.S.OffsetModulatorChain(*self.handles()).step(bits_d, None, flush, iterator)

    def sequence(self, bits_d, flush=False, iterator=False):
        y = self.up.step(self.mapper.step(bits_d), None, flush, iterator)
        return self.mixer.step(self.stagger.step(y))

    def state(self):
        return self.mapper.state(), self.stagger.state().tolist(), self.mixer.state()[:2]

    def bits_for(self, n_sym):
        return n_sym * (2 if self.kind == M.QPSK else 1)


def same_state(a: Chain, b: Chain, seed=99):
    """Mapper state, carry, mixer phase, and the interpolator's history as a
    further flushing step shows it (on clones, so a and b stay as they are)."""
    assert a.state() == b.state()
    a2, b2 = a.clone(), b.clone()
    bits = dev(random_bits(a.bits_for(40), seed))
    assert np.array_equal(a2.sequence(bits, True).cpu().numpy(), b2.sequence(bits, True).cpu().numpy())
    assert a2.state() == b2.state()


def stats_delta(S, fn):
    s0 = S.modulate_offset_stats()
    r = fn()
    return r, tuple(b - a for a, b in zip(s0, S.modulate_offset_stats()))


# ----------------------------------------------------------------- goldens
MAN, ARR = G.load_golden()


@pytest.mark.parametrize("chain", MAN["chains"], ids=[c["key"] for c in MAN["chains"]])
def test_chain_goldens(S, chain):
    k = chain["key"]
    ch = Chain(S, chain["kind"], ARR[k + "_taps"], chain["L"], chain["D"], chain["freq"], N=chain["N"])
    bits, pos, ys = ARR[k + "_bits"], 0, []
    for n, flush in zip(chain["calls"], chain["flush"]):
        bd = dev(bits[pos:pos + n])  # its own allocation: 16-byte aligned
        y, d = stats_delta(S, lambda: ch.fused(bd, flush))
        assert d == (1, 0, 0, 0)
        ys.append(y.cpu().numpy())
        pos += n
    assert np.array_equal(np.concatenate(ys), ARR[k + "_out"])
    assert ch.state() == (chain["mapper_state"], ARR[k + "_carry"].tolist(),
                          (chain["mixer_phase"], ch.mixer.state()[1]))


# -------------------------- fused = the sequence = the model and oracle composition
N_SYM = (1, 7, 511, 512, 513, 2047, 2048, 2049, 4101)
# (4, 16), (8, 64): H = 4 / 8 taps per phase, 2 / 4 pairs, the run-time kernels of L = 4 and 8; (4, 128), (2, 32):
# 16 / 8 pairs compiled in; (3, 15): run-time L
SHAPES = [(4, 16, 2), (4, 128, 2), (8, 64, 4), (8, 64, 1), (8, 64, 8), (3, 15, 1), (2, 32, 1)]
WARM = 100


@pytest.mark.parametrize("L,ntaps,D", SHAPES)
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_fused_equals_the_sequence_and_the_model(S, O, kind, L, ntaps, D):
    c = taps(L, ntaps)
    base = Chain(S, kind, c, L, D, 0.1137, state=3)
    warm = random_bits(base.bits_for(WARM), 1)
    base.sequence(dev(warm))  # a history, a carry, a phase, a state to start from
    for k, n_sym in enumerate(N_SYM):
        bits = random_bits(base.bits_for(n_sym), 10 + k)
        bd = dev(bits)
        for flush in (False, True):
            a, b = base.clone(), base.clone()
            y, d = stats_delta(S, lambda: a.fused(bd, flush))
            assert d == (1, 0, 0, 0), "the fused kernel serves these shapes"
            want = b.sequence(bd, flush)
            assert y.shape == want.shape and np.array_equal(y.cpu().numpy(), want.cpu().numpy()), (n_sym, flush)
            same_state(a, b)
            mapper, stag = M.MapperModel(kind, 3), G.StaggerModel(D)
            end = {}
            ref = G.offset_chain(O["strict"], mapper, c, L, stag, 0.1137, [(warm, False), (bits, flush)], end=end)
            assert np.array_equal(y.cpu().numpy(), ref[L * WARM:]), (n_sym, flush)
            assert a.state() == (mapper.state, stag.carry.tolist(), end["mixer"])


def test_iterator_form(S, O):
    """iterator = 1 (upsampling_filters.h:240-323): no output shift."""
    L, D = 4, 2
    c = taps(L, 16) // 64  # small taps: the unshifted sums stay inside int16 mostly, and clamp where not
    for kind in (M.SDPSK, M.QPSK):
        a = Chain(S, kind, c, L, D, -0.2, state=1)
        b = a.clone()
        bd = dev(random_bits(a.bits_for(TI + 9), 5))
        for flush in (False, True):
            y, d = stats_delta(S, lambda: a.fused(bd, flush, True))
            assert d == (1, 0, 0, 0)
            assert np.array_equal(y.cpu().numpy(), b.sequence(bd, flush, True).cpu().numpy())
            same_state(a, b)


# ------------------------------------------------------------------ chunks
# a chunk of 1 symbol; boundaries inside a wave (300, 2348), at a tile edge (2048) and at a wave edge (512)
@pytest.mark.parametrize("cuts", [(300, 2000), (1, 2047, 300), (512, 1, 1536), (2048, 2048)],
                         ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_stream_in_chunks_equals_one_call(S, kind, cuts):
    c = taps(8, 64)
    one = Chain(S, kind, c, 8, 4, -0.3021, state=2)
    parts = one.clone()
    bits = random_bits(one.bits_for(sum(cuts)), 4)
    whole = one.fused(dev(bits), True).cpu().numpy()
    ys, pos = [], 0
    for i, n_sym in enumerate(cuts):
        n = one.bits_for(n_sym)
        bd = dev(bits[pos:pos + n])  # its own allocation: 16-byte aligned, the fused kernel every time
        y, d = stats_delta(S, lambda: parts.fused(bd, i == len(cuts) - 1))
        assert d == (1, 0, 0, 0)
        ys.append(y.cpu().numpy())
        pos += n
    assert np.array_equal(np.concatenate(ys), whole)
    same_state(one, parts)


# ------------------------------------------------------------- sequence path
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_sequence_path_serves_what_the_fused_kernel_does_not(S, O, kind):
    n_sym, L = TI + 7, 4
    bits = random_bits(2 * n_sym + 16, 6)
    # D = L + 1, against the four calls and against the model
    c = taps(L, 16)
    a = Chain(S, kind, c, L, L + 1, 0.1137, state=1)
    b = a.clone()
    nb = a.bits_for(n_sym)
    bd = dev(bits[:nb])
    mapper, stag, calls = M.MapperModel(kind, 1), G.StaggerModel(L + 1), []
    ys = []
    for flush in (False, True):
        y, d = stats_delta(S, lambda: a.fused(bd, flush))
        assert d == (0, 1, 0, 0)
        assert np.array_equal(y.cpu().numpy(), b.sequence(bd, flush).cpu().numpy())
        same_state(a, b)
        ys.append(y.cpu().numpy())
        calls.append((bits[:nb], flush))
    assert np.array_equal(np.concatenate(ys), G.offset_chain(O["strict"], mapper, c, L, stag, 0.1137, calls))
    assert a.state()[:2] == (mapper.state, stag.carry.tolist())
    # int16 taps (variant 1)
    a = Chain(S, kind, c.astype(np.int16), L, 2, 0.1137, state=1, variant=1)
    b = a.clone()
    for flush in (False, True):
        y, d = stats_delta(S, lambda: a.fused(bd, flush))
        assert d == (0, 1, 0, 0)
        assert np.array_equal(y.cpu().numpy(), b.sequence(bd, flush).cpu().numpy())
        same_state(a, b)
    # d_bits off by one byte: the same results as the aligned call
    f, g = Chain(S, kind, c, L, 2, 0.1137, state=1), Chain(S, kind, c, L, 2, 0.1137, state=1)
    whole = dev(bits)
    y, d = stats_delta(S, lambda: f.fused(whole[1:1 + nb], True))
    assert d == (0, 1, 0, 0)
    want, d = stats_delta(S, lambda: g.fused(dev(bits[1:1 + nb]), True))
    assert d == (1, 0, 0, 0)
    assert np.array_equal(y.cpu().numpy(), want.cpu().numpy())
    same_state(f, g)


# --------------------------------------------------------------------- banks
def bank(S, chains, bits_d, bits_stride, out, n_bits, flush):
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles, _ptr, _stream
    A.call("srcdsp_modulate_offset_step_batched", _handles([c.mapper for c in chains]),
           _handles([c.up for c in chains]), _handles([c.stagger for c in chains]),
           _handles([c.mixer for c in chains]), len(chains), C.c_void_p(bits_d.data_ptr()), bits_stride, _ptr(out),
           out.shape[1], n_bits, int(flush), _stream(out))


@pytest.mark.parametrize("shared", [True, False], ids=["shared_bits", "bits_per_row"])
@pytest.mark.parametrize("rows", [3, 65])
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_bank_equals_the_loop(S, kind, rows, shared):
    """65 rows cross kMaxBatch = 64; every row has its own start state,
    carrier, history and carry."""
    import torch
    L, D, n_sym = 4, 2, 300
    c = taps(L, 16)
    chains = [Chain(S, kind, c, L, D, 0.01 * (r + 1), state=r % 4) for r in range(rows)]
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


def test_bank_loop_path_and_python_face(S):
    """Row strides that are no multiple of 16 bytes: the per-channel loop,
    through the Python face, equal to the single calls."""
    import torch
    rows, L, n = 3, 4, 301
    c = taps(L, 16)
    chains = [Chain(S, M.SDPSK, c, L, 2, 0.02 * (r + 1), state=r) for r in range(rows)]
    loop = [ch.clone() for ch in chains]
    bits = random_bits(rows * n, 9).reshape(rows, n)
    out = torch.zeros((rows, L * n, 2), dtype=torch.int16, device="cuda")
    _, d = stats_delta(S, lambda: S.modulate_offset_step_batched(
        [c.mapper for c in chains], [c.up for c in chains], [c.stagger for c in chains], [c.mixer for c in chains],
        dev(bits), out))
    assert d == (0, 0, 0, 1)
    for r in range(rows):
        assert np.array_equal(out[r].cpu().numpy(), loop[r].sequence(dev(bits[r])).cpu().numpy())
        same_state(chains[r], loop[r])
    y = S.modulate_offset_step(*chains[0].handles(), dev(bits[0]))
    assert np.array_equal(y.cpu().numpy(), loop[0].sequence(dev(bits[0])).cpu().numpy())


# ----------------------------------------------------------------- refusals
def test_refusals_leave_every_handle_unchanged(S):
    import torch
    from srcdsp_amd import _capi as A
    c = taps(4, 16)
    chains = [Chain(S, M.QPSK, c, 4, 2, 0.1 * (r + 1), state=r + 1) for r in range(2)]
    for ch in chains:
        ch.sequence(dev(random_bits(64, 2)))
    keep = [ch.clone() for ch in chains]
    a, b = chains
    bd = dev(random_bits(64, 3))
    out = torch.zeros((2, 4 * 32 + 64, 2), dtype=torch.int16, device="cuda")
    st0 = S.modulate_offset_stats()

    def refused(code, fn):
        with pytest.raises(S.SrcdspError) as e:
            fn()
        assert e.value.code == code

    single = S.OffsetModulatorChain(*a.handles())
    refused(A.ERR_SIZE, lambda: single.step(bd, out[0, :4 * 32 + 1]))          # a wrong n_out
    refused(A.ERR_SIZE, lambda: single.step(bd, out[0, :4 * 32], True))        # no room for the flush
    refused(A.ERR_SIZE, lambda: single.step(bd[:63], out[0, :4 * 31]))         # an odd QPSK bit count
    real = S.FilterUpsamplingFir(c, 4, *UP_T[2])
    refused(A.ERR_UNSUPPORTED,
            lambda: S.OffsetModulatorChain(a.mapper, real, a.stagger, a.mixer).step(bd, out[0, :4 * 32]))
    maps, ups, stags, mixers = ([x.mapper for x in chains], [x.up for x in chains], [x.stagger for x in chains],
                                [x.mixer for x in chains])
    go = lambda m, u, g, x, bits=bd, o=out: S.modulate_offset_step_batched(m, u, g, x, bits, o)  # noqa: E731
    refused(A.ERR_ARG, lambda: go([a.mapper, a.mapper], ups, stags, mixers))    # listed twice
    refused(A.ERR_ARG, lambda: go(maps, [a.up, a.up], stags, mixers))
    refused(A.ERR_ARG, lambda: go(maps, ups, [a.stagger, a.stagger], mixers))
    refused(A.ERR_ARG, lambda: go(maps, ups, stags, [b.mixer, b.mixer]))
    refused(A.ERR_ARG, lambda: go([a.mapper, S.SymbolMapperSdpsk()], ups, stags, mixers))             # kinds differ
    refused(A.ERR_ARG, lambda: go(maps, [a.up, S.FilterUpsamplingFir(taps(4, 20), 4, *UP_T[0])], stags, mixers))
    refused(A.ERR_ARG, lambda: go(maps, ups, [a.stagger, S.QStagger(3)], mixers))                     # D differs
    refused(A.ERR_ARG, lambda: go(maps, ups, stags, [a.mixer, S.Mixer(1024)]))                        # N differs
    short = torch.zeros((2, 4 * 32 - 1, 2), dtype=torch.int16, device="cuda")
    refused(A.ERR_SIZE, lambda: go(maps, ups, stags, mixers, o=short))                                 # out_stride short
    refused(A.ERR_SIZE, lambda: go(maps, ups, stags, mixers, bits=bd[:63]))                            # odd QPSK bits
    assert S.modulate_offset_stats() == st0
    for ch, k in zip(chains, keep):
        same_state(ch, k)
