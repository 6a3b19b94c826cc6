"""C transmit chains summed onto one wire in one call
(srcdsp_modulate_sum_step): the call against srcdsp_modulate_offset_step_batched
(staggers = None: srcdsp_modulate_step_batched) into C rows followed by
srcdsp_combine_step on clones, and against tx_chain_model.TxChain rows combined
by combine_model.combine, the wire and all four handles' state of every chain
bit for bit; the clamp is exercised; streams in chunks; the counters say which
path served a call; refusals change no handle.

TI = 2048 symbols is the tile of the fused kernel (one workgroup per tile,
looping over the chains).  Which calls it serves is decided by measurement; the
tests that are about the kernel route every call it takes to it
(srcdsp_modulate_sum_set_min_tiles(1)) and put the measured routing back, the
routing test reads that routing (srcdsp_modulate_sum_geometry)."""
import ctypes as C

import numpy as np
import pytest

import mapper_model as M
from combine_model import combine as combine_model
from test_gpu_modulate_offset import TI, UP_T, Chain, bank, dev, random_bits, same_state, taps
from tx_chain_model import MODULATE, MODULATE_OFFSET, TxChain

gpu = pytest.mark.gpu


@pytest.fixture
def every_tile_count(S):
    """The fused kernel serves whatever it takes, however short the row."""
    S.modulate_sum_set_min_tiles(1)
    yield
    S.modulate_sum_set_min_tiles(0)


def make_chains(S, kind, L, ntaps, D, rows, scale=1, variant=0, same_freq=None):
    c = taps(L, ntaps) // scale
    if variant == 1:
        c = c.astype(np.int16)
    return [Chain(S, kind, c, L, D, same_freq if same_freq is not None else -0.8 + 1.6 * (r + 0.5) / rows,
                  state=r % 4, variant=variant) for r in range(rows)]


def warm(chains, n_sym=40):
    """A history, a carry, a phase and a state to start from, each chain its own."""
    for r, ch in enumerate(chains):
        ch.sequence(dev(random_bits(ch.bits_for(n_sym + r % 5), 100 + r)))


def bits_for(chains, n_sym, shared, seed):
    """(device bits, bits_stride, n_bits): one shared row, or private rows a
    multiple of 16 bytes apart."""
    n = chains[0].bits_for(n_sym)
    if shared:
        return dev(random_bits(max(n, 1), seed))[:n], 0, n
    stride = max((n + 15) // 16 * 16, 16)
    return dev(random_bits(len(chains) * stride, seed).reshape(len(chains), stride)), stride, n


def n_out_of(chains, n_bits, flush):
    up = chains[0].up
    n_sym = n_bits // 2 if chains[0].kind == M.QPSK else n_bits
    return up.L * (n_sym + (up.getLength() // up.L if flush else 0))


def lists(chains, stagger=True):
    return ([c.mapper for c in chains], [c.up for c in chains], [c.stagger for c in chains] if stagger else None,
            [c.mixer for c in chains])


def sum_call(S, chains, bd, stride, n_bits, flush, shift, stagger=True, out=None, n_out=None):
    import torch
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles, _stream
    n_out = n_out_of(chains, n_bits, flush) if n_out is None else n_out
    if out is None:
        out = torch.full((n_out + 4, 2), 77, dtype=torch.int16, device="cuda")  # guard samples behind the row
    maps, ups, stags, mixers = lists(chains, stagger)
    A.call("srcdsp_modulate_sum_step", _handles(maps), _handles(ups), _handles(stags) if stagger else None,
           _handles(mixers), len(chains), C.c_void_p(bd.data_ptr()), stride, C.c_void_p(out.data_ptr()), n_out, n_bits,
           int(flush), shift, _stream(out))
    y = out.cpu().numpy()
    assert (y[n_out:] == 77).all()
    return y[:n_out]


def pair_call(S, chains, bd, stride, n_bits, flush, shift, stagger=True):
    """The bank into C private rows, then the combiner."""
    import torch
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles, _ptr, _stream
    n_out = n_out_of(chains, n_bits, flush)
    rows = torch.zeros((len(chains), (n_out + 7) // 4 * 4, 2), dtype=torch.int16, device="cuda")  # rows 16 bytes apart
    if stagger:
        bank(S, chains, bd, stride, rows, n_bits, flush)
    else:
        maps, ups, _, mixers = lists(chains, False)
        A.call("srcdsp_modulate_step_batched", _handles(maps), _handles(ups), _handles(mixers), len(chains),
               C.c_void_p(bd.data_ptr()), stride, _ptr(rows), rows.shape[1], n_bits, int(flush), _stream(rows))
    return S.combine(rows[:, :n_out], None, shift).cpu().numpy()


def stats_delta(S, fn):
    s0 = S.modulate_sum_stats()
    r = fn()
    return r, tuple(b - a for a, b in zip(s0, S.modulate_sum_stats()))


def fused_serves(L):
    return L in (2, 4, 8)


# ------------------------------------------------ equals bank + combine on clones
N_SYM = (1, 7, 2047, 2048, 2049, 4101)
SHAPES = ((4, 16, 2), (4, 128, 2), (2, 32, 1), (8, 64, 4), (3, 15, 1))
ROWS = (1, 2, 3, 5, 64)
SHIFTS = (0, 2, 15)
# 30 cases: every (n_sym, shape) pair once; rows, kind, shift, shared bits and the stagger cycle at other periods,
# so each of their values meets every shape and every n_sym
CASES = [(N_SYM[i % 6], SHAPES[i % 5], ROWS[(i + i // 5) % 5], (M.SDPSK, M.QPSK)[(i // 5) % 2],
          SHIFTS[(i + i // 6) % 3], (i // 3) % 2 == 0, (i % 7) not in (2, 5)) for i in range(30)]


def test_the_sweep_covers_what_it_names():
    for k, values in enumerate((N_SYM, SHAPES, ROWS, (M.SDPSK, M.QPSK), SHIFTS, (True, False), (True, False))):
        assert {c[k] for c in CASES} == set(values), k
    assert {(c[0], c[1]) for c in CASES} == {(n, s) for n in N_SYM for s in SHAPES}
    for L in (2, 4, 8):  # the fused kernel's shapes meet both mapper kinds, one chain, 64 chains and no stagger
        mine = [c for c in CASES if c[1][0] == L]
        assert {c[3] for c in mine} == {M.SDPSK, M.QPSK} and {c[6] for c in mine} == {True, False}
    assert {c[2] for c in CASES if c[1][0] == 4} >= {1, 64}


@gpu
@pytest.mark.parametrize("n_sym,shape,rows,kind,shift,shared,stagger", CASES,
                         ids=[f"{c[0]}-L{c[1][0]}t{c[1][1]}D{c[1][2]}-C{c[2]}-k{c[3]}-s{c[4]}-"
                              f"{'shared' if c[5] else 'private'}-{'stag' if c[6] else 'nostag'}" for c in CASES])
def test_equals_the_bank_and_the_combiner(S, every_tile_count, n_sym, shape, rows, kind, shift, shared, stagger):
    L, ntaps, D = shape
    base = make_chains(S, kind, L, ntaps, D, rows, scale=min(rows, 4))
    warm(base)
    bd, stride, n_bits = bits_for(base, n_sym, shared, 7 * n_sym + rows)
    for flush in (False, True):
        a, b = [c.clone() for c in base], [c.clone() for c in base]
        y, d = stats_delta(S, lambda: sum_call(S, a, bd, stride, n_bits, flush, shift, stagger))
        assert d == ((1, 0) if fused_serves(L) else (0, 1)), d
        want = pair_call(S, b, bd, stride, n_bits, flush, shift, stagger)
        assert y.shape == want.shape and np.array_equal(y, want), flush
        for x, z in zip(a, b):
            same_state(x, z)
    # the other route of the same call, whatever the threshold: the same wire
    S.modulate_sum_set_min_tiles(1 << 40)
    a = [c.clone() for c in base]
    y2, d = stats_delta(S, lambda: sum_call(S, a, bd, stride, n_bits, True, shift, stagger))
    assert d == (0, 1) and np.array_equal(y2, want)


# --------------------------------------------------------------- equals the model
@gpu
@pytest.mark.parametrize("stagger", [True, False], ids=["offset", "plain"])
@pytest.mark.parametrize("L,ntaps,D", [(4, 16, 2), (2, 32, 1)])
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_equals_the_model(S, O, every_tile_count, kind, L, ntaps, D, stagger):
    rows, n_sym, shift = 3, TI + 1, 1
    c = taps(L, ntaps) // 2
    freqs = [-0.5, 0.1137, 0.7]
    chains = [Chain(S, kind, c, L, D, freqs[r], state=r + 1) for r in range(rows)]
    model = [TxChain(O["strict"], MODULATE_OFFSET if stagger else MODULATE, L, c, 4096, freqs[r], kind,
                     D if stagger else None, mapper_state=r + 1) for r in range(rows)]
    bits = [random_bits(chains[0].bits_for(n), 30 + i).reshape(1, -1).repeat(rows, 0) for i, n in enumerate((100, n_sym))]
    for r in range(rows):  # private rows that differ
        bits[1][r] = np.roll(bits[1][r], 2 * r)
    for i, (b, flush) in enumerate(zip(bits, (False, True))):
        n = b.shape[1]
        stride = (n + 15) // 16 * 16
        padded = np.zeros((rows, stride), np.uint8)
        padded[:, :n] = b
        y, d = stats_delta(S, lambda: sum_call(S, chains, dev(padded), stride, n, flush, shift, stagger))
        assert d == (1, 0)
        want = combine_model(np.stack([model[r].step(b[r], flush) for r in range(rows)]), shift)
        assert np.array_equal(y, want), i
        for r in range(rows):
            st = model[r].state()
            got = chains[r].state()
            assert got[0] == st["mapper"] and got[2] == st["mixer"], (i, r)
            if stagger:
                assert got[1] == st["carry"], (i, r)


# ------------------------------------------------------------------- the clamp
CLAMP = dict(rows=5, L=4, ntaps=16, D=2, n_sym=TI + 9, freq=0.1137)


def clamp_model(o, kind):
    """The unclamped sum of 5 chains on one frequency fed the same bits: 5 x one row."""
    k = CLAMP
    t = TxChain(o, MODULATE_OFFSET, k["L"], taps(k["L"], k["ntaps"]), 4096, k["freq"], kind, k["D"])
    bits = random_bits(k["n_sym"] * (2 if kind == M.QPSK else 1), 55)
    row = t.step(bits)
    return bits, row, k["rows"] * row.astype(np.int64)


@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_the_clamp_case_clips_at_both_ends_and_the_shifted_one_does_not(O, kind):
    """A condition, not a tolerance: the GPU case below cannot pass on an unclipped wire."""
    _, _, total = clamp_model(O["strict"], kind)
    assert total.max() > 32767 and total.min() < -32768, (total.min(), total.max())
    assert (total >> 3).max() <= 32767 and (total >> 3).min() >= -32768


@gpu
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_the_clamp_is_exercised(S, O, every_tile_count, kind):
    k = CLAMP
    bits, row, total = clamp_model(O["strict"], kind)
    bd = dev(bits)
    for shift in (0, 3):
        chains = [Chain(S, kind, taps(k["L"], k["ntaps"]), k["L"], k["D"], k["freq"]) for _ in range(k["rows"])]
        y, d = stats_delta(S, lambda: sum_call(S, chains, bd, 0, len(bits), False, shift))
        assert d == (1, 0)
        assert np.array_equal(y, np.clip(total >> shift, -32768, 32767).astype(np.int16)), shift
        assert np.array_equal(y, combine_model(np.stack([row] * k["rows"]), shift))
        clipped = int((y.astype(np.int64) != total >> shift).sum())
        assert (clipped > 0) == (shift == 0), (shift, clipped)
        if shift == 0:
            assert y.max() == 32767 and y.min() == -32768


# ------------------------------------------------------------------ in chunks
@gpu
@pytest.mark.parametrize("cuts", [(2047, 2, 2049), (2049, 2047, 300)], ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_stream_in_chunks(S, every_tile_count, kind, cuts):
    """Three calls, the last flushing, the chunk ends on either side of a tile
    edge; the bank and the combiner in the same chunks; the states after every
    call.  The chunks together equal one call."""
    rows, L, shift = 3, 4, 1
    a = make_chains(S, kind, L, 128, 2, rows, scale=2)
    warm(a)
    b, one = [c.clone() for c in a], [c.clone() for c in a]
    n_sym = sum(cuts)
    nb = a[0].bits_for(n_sym)
    stride = (nb + 15) // 16 * 16
    bits = random_bits(rows * stride, 9).reshape(rows, stride)
    whole = sum_call(S, one, dev(bits), stride, nb, True, shift)
    ys, pos = [], 0
    for i, cut in enumerate(cuts):
        n = a[0].bits_for(cut)
        cs = (n + 15) // 16 * 16
        part = np.zeros((rows, cs), np.uint8)
        part[:, :n] = bits[:, pos:pos + n]
        bd = dev(part)
        last = i == len(cuts) - 1
        y, d = stats_delta(S, lambda: sum_call(S, a, bd, cs, n, last, shift))
        assert d == (1, 0)
        assert np.array_equal(y, pair_call(S, b, bd, cs, n, last, shift)), i
        for x, z in zip(a, b):
            same_state(x, z)
        ys.append(y)
        pos += n
    assert np.array_equal(np.concatenate(ys), whole)
    for x, z in zip(a, one):
        same_state(x, z)


# -------------------------------------------------------------------- routing
@gpu
@pytest.mark.parametrize("L,ntaps,D", [(4, 16, 2), (2, 32, 1), (8, 64, 4)])
def test_the_measured_routing(S, L, ntaps, D):
    """Where the measured routing names calls at this L (srcdsp_modulate_sum_geometry),
    the fused kernel serves the call at the threshold, and the bank and the
    combiner serve it one tile below and with one chain too many; where it names
    none, they serve every call.  The results are the same."""
    tile, need, most = S.modulate_sum_geometry(L)
    assert tile == TI
    if need == 0:
        cases = [(2 * TI + 5, 2, (0, 1))]
    else:
        cases = [((need - 1) * TI + 1, 2, (1, 0)), ((need - 1) * TI, 2, (0, 1)), ((need - 1) * TI + 1, most + 1, (0, 1))]
    for n_sym, rows, route in cases:
        base = make_chains(S, M.QPSK, L, ntaps, D, rows, scale=2)
        bd, stride, n_bits = bits_for(base, n_sym, True, 3)
        a, b = [c.clone() for c in base], [c.clone() for c in base]
        y, d = stats_delta(S, lambda: sum_call(S, a, bd, stride, n_bits, False, 2))
        assert d == route, (n_sym, rows, d)
        assert np.array_equal(y, pair_call(S, b, bd, stride, n_bits, False, 2))
        for x, z in zip(a, b):
            assert x.state() == z.state()
        same_state(a[1], b[1])


@gpu
@pytest.mark.parametrize("why", ["65_chains", "D_above_L", "int16_taps", "odd_address", "bits_stride", "short_row",
                                 "L_5", "L_3"])
def test_what_the_fused_kernel_does_not_take_goes_to_the_bank(S, why):
    """With identical results.  Every case but `short_row` runs with the
    threshold at one tile, so the named reason alone decides."""
    import torch
    L, ntaps, D, rows, variant = 4, 16, 2, 3, 0
    if why == "65_chains":
        rows = 65
    elif why == "D_above_L":
        D = 5
    elif why == "int16_taps":
        variant = 1
    elif why == "L_5":
        L, ntaps, D = 5, 40, 2
    elif why == "L_3":
        L, ntaps, D = 3, 15, 1
    n_sym = 4101
    base = make_chains(S, M.QPSK, L, ntaps, D, rows, scale=4, variant=variant)
    warm(base)
    n = base[0].bits_for(n_sym)
    if why == "odd_address":
        whole = dev(random_bits(n + 16, 5))
        bd, stride = whole[1:1 + n], 0
    elif why == "bits_stride":
        stride = n + 8  # rows 8 bytes off a multiple of 16
        bd = dev(random_bits(rows * stride, 5).reshape(rows, stride))
    else:
        bd, stride, _ = bits_for(base, n_sym, why != "65_chains", 5)
    S.modulate_sum_set_min_tiles(0 if why == "short_row" else 1)
    try:
        a, b = [c.clone() for c in base], [c.clone() for c in base]
        y, d = stats_delta(S, lambda: sum_call(S, a, bd, stride, n, True, 2))
        assert d == (0, 1), d
        if why == "odd_address":
            bd = bd.clone()  # its own allocation: the bank's one launch serves the reference
        assert np.array_equal(y, pair_call(S, b, bd, stride, n, True, 2))
        for x, z in zip(a, b):
            assert x.state() == z.state()
        for r in (0, rows - 1):
            same_state(a[r], b[r])
        if why in ("odd_address", "bits_stride", "short_row"):  # the fused kernel on the same bits: the same wire
            S.modulate_sum_set_min_tiles(1)
            f = [c.clone() for c in base]
            if why == "bits_stride":
                s2 = (n + 15) // 16 * 16
                wide = torch.zeros((rows, s2), dtype=torch.uint8, device="cuda")
                wide[:, :n] = bd[:, :n]
                bd, stride = wide, s2
            y2, d = stats_delta(S, lambda: sum_call(S, f, bd, stride, n, True, 2))
            assert d == (1, 0) and np.array_equal(y2, y)
    finally:
        S.modulate_sum_set_min_tiles(0)


@gpu
def test_python_face(S, every_tile_count):
    """out made by the call, a [C, n] view of wider bit rows, staggers=None."""
    rows, L, n_sym = 3, 4, TI + 5
    base = make_chains(S, M.SDPSK, L, 16, 2, rows, scale=2)
    bd, stride, n = bits_for(base, n_sym, False, 8)
    for stagger in (True, False):
        a, b = [c.clone() for c in base], [c.clone() for c in base]
        y, d = stats_delta(S, lambda: S.modulate_sum_step(*lists(a, stagger), bd[:, :n], None, 2, True))
        assert d == (1, 0) and tuple(y.shape) == (n_out_of(a, n, True), 2)
        assert np.array_equal(y.cpu().numpy(), pair_call(S, b, bd, stride, n, True, 2, stagger))
        out = S.modulate_sum_step(*lists(a, stagger), bd[0, :n], y[:L * n_sym], shift=2)  # shared bits, out given
        assert out.data_ptr() == y.data_ptr()
        assert np.array_equal(out.cpu().numpy(), pair_call(S, b, bd[0, :n].clone(), 0, n, False, 2, stagger))
        for x, z in zip(a, b):
            same_state(x, z)


# ------------------------------------------------------------------- refusals
@gpu
def test_refusals_leave_every_handle_unchanged(S):
    import torch
    from srcdsp_amd import _capi as A
    L, n_sym = 4, 32
    chains = make_chains(S, M.QPSK, L, 16, 2, 2)
    warm(chains)
    keep = [c.clone() for c in chains]
    a, b = chains
    bd = dev(random_bits(2 * n_sym, 3))
    out = torch.full((L * n_sym + 64, 2), 77, dtype=torch.int16, device="cuda")
    st0 = S.modulate_sum_stats()

    def refused(code, fn):
        with pytest.raises(S.SrcdspError) as e:
            fn()
        assert e.value.code == code
        assert S.modulate_sum_stats() == st0
        assert (out == 77).all()
        for ch, k in zip(chains, keep):
            same_state(ch, k)

    def go(group=None, bits=bd, n_bits=2 * n_sym, n_out=L * n_sym, shift=0, flush=False, o=out, stagger=True):
        sum_call(S, group or chains, bits, 0, n_bits, flush, shift, stagger, out=o, n_out=n_out)

    c16 = taps(L, 16)
    other_kind = Chain(S, M.SDPSK, c16, L, 2, 0.3)
    other_L = Chain(S, M.QPSK, taps(2, 16), 2, 2, 0.3)
    other_taps = Chain(S, M.QPSK, taps(L, 20), L, 2, 0.3)
    other_D = Chain(S, M.QPSK, c16, L, 3, 0.3)
    other_N = Chain(S, M.QPSK, c16, L, 2, 0.3, N=1024)
    for who in (other_kind, other_L, other_taps, other_D, other_N):
        refused(A.ERR_ARG, lambda: go([a, who]))
    refused(A.ERR_ARG, lambda: go([a, other_kind], stagger=False))
    for attr in ("mapper", "up", "stagger", "mixer"):  # a handle listed twice
        twin = b.clone()
        setattr(twin, attr, getattr(a, attr))
        refused(A.ERR_ARG, lambda: go([a, twin]))
    refused(A.ERR_ARG, lambda: go(shift=16))
    refused(A.ERR_SIZE, lambda: go(n_out=L * n_sym + 1))       # a wrong n_out: longer,
    refused(A.ERR_SIZE, lambda: go(n_out=L * n_sym - 1))       # shorter,
    refused(A.ERR_SIZE, lambda: go(flush=True, n_out=L * n_sym))  # no room for the flush
    refused(A.ERR_SIZE, lambda: go(n_bits=2 * n_sym - 1, n_out=L * (n_sym - 1)))  # an odd QPSK n_bits

    def null_out():
        from srcdsp_amd.operators import _handles, _stream
        maps, ups, stags, mixers = lists(chains)
        A.call("srcdsp_modulate_sum_step", _handles(maps), _handles(ups), _handles(stags), _handles(mixers), 2,
               C.c_void_p(bd.data_ptr()), 0, None, L * n_sym, 2 * n_sym, 0, 0, _stream(bd))

    refused(A.ERR_ARG, null_out)
    real = Chain(S, M.QPSK, c16, L, 2, 0.3, variant=2)
    refused(A.ERR_UNSUPPORTED, lambda: go([real]))
    # n_out == 0 does nothing
    go(bits=bd[:0], n_bits=0, n_out=0)
    assert S.modulate_sum_stats() == st0
    for ch, k in zip(chains, keep):
        same_state(ch, k)
