"""srcdsp_demod_*: the OQPSK demodulator on the GPU, single step and bank.
Everything is integer, so every comparison is bit for bit: against the goldens
recorded from the reference (tests/golden/demod_golden.*) and, for shapes the
goldens do not hold, against tests/demod_model.py, which
tests/test_demod_model_golden.py pins to the same goldens.  T = 64 is the
kernel's tile (samples per row and tile), 64 rows a workgroup."""
import ctypes as C

import numpy as np
import pytest

import demod_model as M

pytestmark = pytest.mark.gpu

MAN, ARR = M.load_golden()
T = MAN["tile"]
N_BANK = 2 * T + 5
PS = (0, 2, 16, T + 3)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def pair(S, P, shift, word, seed, ref_len=None):
    """A demodulator and the model, configured alike with a random pattern and
    reference (the order of tests/cpp/demod_main.cpp)."""
    rng = np.random.default_rng(seed)
    g, m = S.DemodulatorOqpsk(), M.DemodModel()
    bits = rng.integers(0, 2, P).astype(np.int8)
    ref = rng.integers(-16000, 16001, size=(P if ref_len is None else ref_len, 2)).astype(np.int16)
    f = M.word_freq(word)
    for d in (g, m):
        if P:
            d.set_sync_pattern(bits)
        d.set_reference(ref)
        d.set_initial_frequency(float(f))
        d.reset()
        d.set_input_shift(shift)
    return g, m


def noise(seed, shape, amp=16000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, size=shape + (2,)).astype(np.int16)


def same(g, m, tag):
    assert g.state() == m.state(), tag
    assert np.float32(g.getMeasuredFrequency()).tobytes() == m.measured_frequency().tobytes(), tag


# ------------------------------------------------------ group 1: parity, state
def test_library_tables_equal_the_golden_tables(S):
    """Built by the host libm of this machine with the reference's expressions."""
    s, p = S.demod_tables()
    assert np.array_equal(s, ARR["sine"]) and np.array_equal(p, ARR["phase"])


@pytest.mark.parametrize("key", [c["key"] for c in MAN["cases"]])
def test_golden_case(S, key):
    """Soft bits, error and measured frequency of every call as the reference
    wrote them, through srcdsp_demod_step and srcdsp_demod_step_host; the
    state against the model after every call."""
    case = next(c for c in MAN["cases"] if c["key"] == key)
    x = ARR[key + "_x"]
    for device in (True, False):
        g, m = S.DemodulatorOqpsk(), M.golden_case_model(case, ARR)
        if case["P"]:
            g.setSyncPattern(ARR[key + "_bits"])
        g.setReference(ARR[key + "_ref"])
        g.setInitialFrequency(float(ARR[key + "_freq"][0]))
        g.reset()
        g.setInputShift(case["shift"])
        pos = spos = 0
        for i, n in enumerate(case["chunks"]):
            if i == case["reset_before"]:
                g.reset()
                m.reset()
                assert g.state()[9] == 0
            chunk = x[pos:pos + n]
            soft, err = g.step(dev(chunk) if device else chunk)
            soft = soft.cpu().numpy() if device else soft
            m.step(chunk)
            pos += n
            ns = case["soft_sizes"][i]
            tag = (key, device, i)
            assert soft.dtype == np.int8 and len(soft) == ns, tag
            assert np.array_equal(soft, ARR[key + "_soft"][spos:spos + ns]), tag
            spos += ns
            assert err == ARR[key + "_error"][i], tag
            assert np.float32(g.getMeasuredFrequency()).tobytes() == ARR[key + "_mfreq"][i].tobytes(), tag
            same(g, m, tag)


def test_clone_continues_bit_for_bit(S):
    import copy
    g, m = pair(S, 16, 3, -13, 1)
    x = noise(2, (3 * T + 9,))
    g.step(dev(x[:T + 7]))
    m.step(x[:T + 7])
    c = copy.copy(g)
    same(c, m, "clone")
    want, werr = m.step(x[T + 7:])
    for d in (g, c):  # the original and the copy continue alike, independently
        soft, err = d.step(dev(x[T + 7:]))
        assert np.array_equal(soft.cpu().numpy(), want) and err == werr
        same(d, m, "after")


def test_reset_behaves_as_the_reference(S):
    """demodulators.cpp:293-308: StateVar cleared, the shift back to 0, bit1 and
    bit2 from the last two sync bits; the next call is a first call again."""
    g, m = pair(S, 16, 5, 13, 3)
    x = noise(4, (T + 20,), amp=32767)
    g.step(dev(x))
    m.step(x)
    assert g.state()[9] == 5
    g.reset()
    m.reset()
    st = g.state()
    assert st[9] == 0 and st[0] == 0 and st[3] in (-1, 1) and st[4] in (-1, 1)
    same(g, m, "reset")
    soft, err = g.step(dev(x))
    want, werr = m.step(x)
    assert len(soft) == len(x) - 16 and np.array_equal(soft.cpu().numpy(), want) and err == werr
    same(g, m, "after reset")


# --------------------------------------------------- group 2: bank, refusals
def bank_pairs(S, channels, seed0=100):
    """Per channel its own P, shift, frequency word, pattern and reference;
    every second one already stepped once (a prior state)."""
    words = (0, 13, -13, 4096, -4096, 500, -777)
    out = []
    for c in range(channels):
        g, m = pair(S, PS[c % 4], (0, 3, 8, 1, 6)[c % 5], words[c % 7], seed0 + c)
        if c % 2:
            pre = noise(5000 + c, (T + 6 + c % 3,))
            g.step(pre)
            m.step(pre)
        out.append((g, m))
    return out


@pytest.mark.parametrize("channels", [1, 2, 63, 64, 65, 130])
def test_bank_equals_the_loop_and_the_model(S, channels):
    """channels across the wave and the workgroup, n = 2 T + 5: the bank call,
    the loop of single steps on clones, and the model agree in soft bits,
    n_soft, error and the state every handle is left with."""
    import copy
    ps = bank_pairs(S, channels)
    x = noise(7, (channels, N_BANK), amp=20000)
    xd = dev(x)
    loop = [copy.copy(g) for g, _ in ps]
    soft, ns, errs = S.demod_step_batched([g for g, _ in ps], xd)
    soft = soft.cpu().numpy()
    for c, (g, m) in enumerate(ps):
        want, werr = m.step(x[c])
        ls, lerr = loop[c].step(xd[c])
        assert ns[c] == len(want) == len(ls), c
        assert np.array_equal(soft[c, :ns[c]], want) and np.array_equal(ls.cpu().numpy(), want), c
        assert errs[c] == werr == lerr, c
        same(g, m, c)
        same(loop[c], m, c)


def test_shared_input_frequency_hypotheses(S):
    """in_stride == 0: five frequency words on one burst."""
    words = (0, 13, -13, 4096, -4096)
    x = noise(8, (N_BANK,))
    ps = []
    for w in words:
        g, m = pair(S, 16, 2, w, 9)  # the same pattern and reference, another word
        ps.append((g, m))
    soft, ns, errs = S.demod_step_batched([g for g, _ in ps], dev(x))
    soft = soft.cpu().numpy()
    outs = []
    for c, (g, m) in enumerate(ps):
        want, werr = m.step(x)
        assert ns[c] == len(want) and np.array_equal(soft[c, :ns[c]], want) and errs[c] == werr, c
        same(g, m, c)
        outs.append(want.tobytes())
    # the hypotheses do differ -- but for +-4096: a step of +pi and one of -pi
    # are the same phase modulo 8192 (their accumulated frequencies differ)
    assert len(set(outs)) == 4 and outs[3] == outs[4]
    assert ps[3][0].state()[8] != ps[4][0].state()[8]


def test_odd_input_offsets(S):
    """in_offset odd: rows that start at samples 1, 3, 5, ... are 4-byte but
    not 16-byte aligned."""
    channels = 6
    ps = bank_pairs(S, channels, seed0=300)
    offs = [2 * c + 1 for c in range(channels)]
    x = noise(10, (channels, N_BANK + max(offs)))
    soft, ns, errs = S.demod_step_batched([g for g, _ in ps], dev(x), offsets=offs, n=N_BANK)
    soft = soft.cpu().numpy()
    for c, (g, m) in enumerate(ps):
        want, werr = m.step(x[c, offs[c]:offs[c] + N_BANK])
        assert ns[c] == len(want) and np.array_equal(soft[c, :ns[c]], want) and errs[c] == werr, c
        same(g, m, c)


def test_bank_and_single_steps_continue_each_other(S):
    channels = 5
    ps = bank_pairs(S, channels, seed0=400)
    gs = [g for g, _ in ps]
    x = noise(11, (channels, 3 * N_BANK))
    xd = dev(x)

    def single(lo, hi):
        for c, (g, m) in enumerate(ps):
            soft, err = g.step(xd[c, lo:hi])
            want, werr = m.step(x[c, lo:hi])
            assert np.array_equal(soft.cpu().numpy(), want) and err == werr, (c, lo)
            same(g, m, (c, lo))

    def bank(lo, hi):
        soft, ns, errs = S.demod_step_batched(gs, xd[:, lo:hi].contiguous())
        soft = soft.cpu().numpy()
        for c, (g, m) in enumerate(ps):
            want, werr = m.step(x[c, lo:hi])
            assert ns[c] == len(want) and np.array_equal(soft[c, :ns[c]], want) and errs[c] == werr, (c, lo)
            same(g, m, (c, lo))

    bank(0, N_BANK)
    single(N_BANK, 2 * N_BANK)
    bank(2 * N_BANK, 3 * N_BANK)


def test_lead_scratch_grows_and_is_reused(S):
    """The table and the result rows live on hs[0] and only grow: one lead
    through calls of 2, 5 and 2 channels (kept, regrown, reused at the larger
    capacity), each call against the loop of single steps on clones."""
    import copy
    gs = [pair(S, 32, c % 3, (13, -13, 500, 0, -777)[c], 600 + c)[0] for c in range(5)]
    for call, ch in enumerate((2, 5, 2)):
        xd = dev(noise(20 + call, (ch, 512)))
        loop = [copy.copy(g) for g in gs[:ch]]
        soft, ns, errs = S.demod_step_batched(gs[:ch], xd)
        soft = soft.cpu().numpy()
        for c in range(ch):
            ls, lerr = loop[c].step(xd[c])
            first = call == (0 if c < 2 else 1)  # a handle's first call keeps the 32 preamble bits back
            assert ns[c] == len(ls) == (512 - 32 if first else 512), (call, c)
            assert np.array_equal(soft[c, :ns[c]], ls.cpu().numpy()) and errs[c] == lerr, (call, c)
            assert gs[c].state() == loop[c].state(), (call, c)
            assert np.float32(gs[c].getMeasuredFrequency()).tobytes() == \
                np.float32(loop[c].getMeasuredFrequency()).tobytes(), (call, c)


def test_refusals_change_no_handle(S):
    from srcdsp_amd import _capi as A
    lib = A.lib()
    g, m = pair(S, 16, 2, 13, 500)
    short, _ = pair(S, 16, 0, 0, 501, ref_len=7)  # a reference shorter than the preamble
    other, _ = pair(S, 0, 0, 0, 502)
    x = dev(noise(12, (2, N_BANK)))
    soft = dev(np.zeros((2, N_BANK), np.int8))
    ns, err = (C.c_size_t * 2)(9, 9), (C.c_int32 * 2)(9, 9)
    before = [d.state() for d in (g, short, other)]

    def batched(hs, n, stride):
        arr = (C.c_void_p * len(hs))(*[h._h.value for h in hs])
        return lib.srcdsp_demod_step_batched(arr, len(hs), C.c_void_p(x.data_ptr()), N_BANK, None, n,
                                             C.c_void_p(soft.data_ptr()), stride, ns, err, None)

    one = C.c_size_t(9)
    e1 = C.c_int32(9)
    # cap too small: the first call of g returns N_BANK - 16 soft bits
    assert lib.srcdsp_demod_step(g._h, C.c_void_p(x.data_ptr()), N_BANK, C.c_void_p(soft.data_ptr()), N_BANK - 17,
                                 C.byref(one), C.byref(e1), None) == A.ERR_SIZE
    assert batched([other, g], N_BANK, N_BANK - 1) == A.ERR_SIZE       # other needs N_BANK
    assert batched([other, g], 16, N_BANK) == A.ERR_SIZE               # n <= P on g's first call
    assert batched([other, short], N_BANK, N_BANK) == A.ERR_SIZE       # 7 reference samples, 15 read
    assert batched([g, other, g], N_BANK, N_BANK) == A.ERR_ARG         # a handle listed twice
    assert [d.state() for d in (g, short, other)] == before
    assert (one.value, e1.value, list(ns), list(err)) == (9, 9, [9, 9], [9, 9])
    assert not soft.any().item()
    # and the handles still step as if nothing had been asked
    got, gerr = g.step(x[0])
    want, werr = m.step(x[0].cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), want) and gerr == werr
    same(g, m, "after the refusals")
