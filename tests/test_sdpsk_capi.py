"""CPU-side checks of the SDPSK demodulator (srcdsp_sdpsk_*): the numpy model
against the definition; the mapper round trip; exported, in the ctypes
signature table and the header; the argument rules that refuse a call before
any HIP call; srcdsp_sdpsk_step_host against the model; the kernel's arithmetic
run on the host under sanitisers; the C++ drop-in; the kernel's gfx950
resources -- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mapper_model import SDPSK, MapperModel
from sdpsk_model import SdpskModel, soft_of, tq_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_sdpsk_create", "srcdsp_sdpsk_destroy", "srcdsp_sdpsk_clone", "srcdsp_sdpsk_reset",
       "srcdsp_sdpsk_set_shift", "srcdsp_sdpsk_get_state", "srcdsp_sdpsk_geometry", "srcdsp_sdpsk_step",
       "srcdsp_sdpsk_step_host", "srcdsp_sdpsk_step_batched")
DUMMY = C.c_void_p(4096)    # never dereferenced: every call it goes to is refused, or has nothing to do
DUMMY2 = C.c_void_p(1 << 20)
DS = (1, 2, 3, 4, 63, 64)
TQ_MAX = 2 ** 31 - 32768
# a, b whose tq is the largest and the smallest there is
EXTREME = (((-32768, -32768), (-32768, 32767)), ((-32768, -32768), (32767, -32768)))


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def samples(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, 2)).astype(np.int16)


class Handle:
    def __init__(self, capi, D, shift=0):
        self.capi, self.lib, self.D = capi, capi.lib(), D
        self.h = C.c_void_p()
        assert self.lib.srcdsp_sdpsk_create(C.byref(self.h), D, shift) == 0

    def __del__(self):
        self.lib.srcdsp_sdpsk_destroy(self.h)

    def clone(self):
        c = object.__new__(Handle)
        c.capi, c.lib, c.D, c.h = self.capi, self.lib, self.D, C.c_void_p()
        assert self.lib.srcdsp_sdpsk_clone(self.h, C.byref(c.h)) == 0
        return c

    def reset(self):
        assert self.lib.srcdsp_sdpsk_reset(self.h) == 0

    def state(self):
        d, s = C.c_uint(), C.c_uint()
        carry = np.full((self.D + 1, 2), 77, np.int16)  # one guard sample
        assert self.lib.srcdsp_sdpsk_get_state(self.h, C.byref(d), C.byref(s), carry.ctypes.data_as(self.capi.I16P)) == 0
        assert (carry[-1] == 77).all()
        return d.value, s.value, carry[:-1]

    def step(self, x, soft=True, bits=True):
        """srcdsp_sdpsk_step_host; one guard byte after each output."""
        x = np.ascontiguousarray(x, np.int16)
        n = len(x)
        s, b = np.full(n + 1, 77, np.int8), np.full(n + 1, 77, np.uint8)
        assert self.lib.srcdsp_sdpsk_step_host(self.h, x.ctypes.data, n, s.ctypes.data if soft else None,
                                               b.ctypes.data if bits else None) == 0
        assert s[-1] == 77 and b[-1] == 77
        return s[:-1], b[:-1]


# ------------------------------------------------------------------- the model
def test_model_definition():
    """The numpy model against the definition written out component by component."""
    x = samples(50, 1)
    for D, shift in ((1, 0), (3, 17), (64, 31)):
        m = SdpskModel(D, shift, samples(D, 2))
        v = [tuple(int(c) for c in s) for s in np.concatenate([m.carry, x])]
        soft, bits = m.step(x)
        for i in range(50):
            (ar, ai), (br, bi) = v[i + D], v[i]
            tq = ai * br - ar * bi
            s = tq >> shift
            assert soft[i] == (127 if s > 127 else -128 if s < -128 else s)
            assert bits[i] == (1 if tq > 0 else 0)
        assert m.carry.tolist() == [list(s) for s in v[50:50 + D]]
    m = SdpskModel(4, 0, samples(4, 3))  # n < D: the carry keeps its tail
    c0 = m.carry.copy()
    m.step(x[:3])
    assert np.array_equal(m.carry, np.concatenate([c0[3:], x[:3]]))


def test_model_extremes_and_clamps():
    (a0, b0), (a1, b1) = EXTREME
    assert tq_of(a0, b0) == TQ_MAX and tq_of(a1, b1) == -TQ_MAX
    for (a, b), sign in zip(EXTREME, (1, -1)):
        m = SdpskModel(1, 0, [b])
        soft, bits = m.step([a])
        assert soft[0] == (127 if sign > 0 else -128) and bits[0] == (1 if sign > 0 else 0)
    # both clamp ends, and the values next to them, at shift 0 and shift 24
    for shift in (0, 24):
        for t, want in ((127 << shift, 127), (128 << shift, 127), (-128 << shift, -128), ((-129) << shift, -128),
                        ((-128 << shift) - 1, -128), (126 << shift, 126), (-127 << shift, -127)):
            assert soft_of(t, shift) == want, (shift, t)
    assert soft_of(TQ_MAX, 24) == 127 and soft_of(-TQ_MAX, 24) == -128
    assert soft_of(TQ_MAX, 31) == 0 and soft_of(-TQ_MAX, 31) == -1
    # tq == 0 is bit 0: a sample against itself, and against zero
    m = SdpskModel(1, 0, [(1234, -777)])
    soft, bits = m.step([(1234, -777), (0, 0), (5, 5)])
    assert soft.tolist() == [0, 0, 0] and bits.tolist() == [0, 0, 0]


@pytest.mark.parametrize("state", range(4))
def test_mapper_round_trip(state):
    """Bits in equal bits out with no filters: the model at D = 1 over the
    SDPSK mapper's symbols, from any mapper state.  The symbols turn by +-90
    degrees at amplitude 8192, so tq = +-2^27 and shift 20 gives +-128 before
    the clamp: exactly +127 and -128."""
    for seed in range(5):
        bits = np.random.default_rng(100 * state + seed).integers(0, 3, 300).astype(np.uint8)  # 2 counts as a one
        sym = MapperModel(SDPSK, state).step(bits)
        soft, out = SdpskModel(1, 20).step(sym)
        assert np.array_equal(out[1:], (bits[1:] > 0).astype(np.uint8))
        assert np.array_equal(soft[1:], np.where(bits[1:] > 0, 127, -128))
        assert set(soft[1:].tolist()) == {127, -128}
        assert soft[0] == 0 and out[0] == 0  # against the zero carry


# ------------------------------------------------------------------- the C ABI
def test_library_exports_the_new_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_sdpsk_step"][1]) == 6
    assert len(capi.SIGNATURES["srcdsp_sdpsk_step_host"][1]) == 5
    assert len(capi.SIGNATURES["srcdsp_sdpsk_step_batched"][1]) == 11
    with open(capi.HEADER) as f:
        text = f.read()
    assert text.index("DemodulatorOqpsk<int16_t>   (demodulators.h") < text.index("The differential SDPSK demodulator")
    sec = text[text.index("The differential SDPSK demodulator"):text.index("estimateFreq<int16_t, L>   (")]
    assert sec.count("Extension") >= len(NEW)
    assert sec.count("modulators.h:82-131") >= len(NEW) and sec.count("dsp_complex.h:45-63") >= len(NEW)
    assert "before any HIP call and changes no handle" in sec and "drop D outputs" in sec


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("DemodulatorSdpsk", "sdpsk_step_batched", "sdpsk_geometry"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name))


def test_geometry_makes_no_device_call(capi):
    t, d, w = C.c_int(), C.c_uint(), C.c_int(-1)
    assert capi.lib().srcdsp_sdpsk_geometry(C.byref(t), C.byref(d), C.byref(w)) == 0
    assert t.value in (1024, 2048, 4096) and d.value == 64 and w.value == 0
    assert capi.lib().srcdsp_sdpsk_geometry(None, None, None) == 0


def test_refusals_come_before_any_device_call(capi):
    lib = capi.lib()
    h = C.c_void_p(1)
    for D, shift in ((0, 0), (65, 0), (1, 32)):
        assert lib.srcdsp_sdpsk_create(C.byref(h), D, shift) == capi.ERR_ARG and not h.value
    assert lib.srcdsp_sdpsk_create(None, 1, 0) == capi.ERR_ARG
    a, b, c = Handle(capi, 2, 5), Handle(capi, 2, 5), Handle(capi, 3, 5)
    before = [x.state() for x in (a, b, c)]
    assert lib.srcdsp_sdpsk_set_shift(a.h, 32) == capi.ERR_ARG and b"shift" in lib.srcdsp_last_error()
    assert lib.srcdsp_sdpsk_set_shift(None, 1) == capi.ERR_ARG
    # single steps: a null handle, a null input, both outputs null
    for fn, tail in ((lib.srcdsp_sdpsk_step, (None,)), (lib.srcdsp_sdpsk_step_host, ())):
        assert fn(None, DUMMY, 8, DUMMY2, None, *tail) == capi.ERR_ARG
        assert fn(a.h, None, 8, DUMMY2, None, *tail) == capi.ERR_ARG
        assert fn(a.h, DUMMY, 8, None, None, *tail) == capi.ERR_ARG
        assert b"null buffer" in lib.srcdsp_last_error()
        assert fn(a.h, None, 0, None, None, *tail) == capi.OK  # no samples: nothing happens
    # the bank
    def bank(hs, n=8, d_in=DUMMY, soft=DUMMY2, ss=8, bits=None, bs=0, off=None):
        arr = (C.c_void_p * len(hs))(*[x.h.value if x is not None else None for x in hs])
        return lib.srcdsp_sdpsk_step_batched(arr, len(hs), d_in, 8, off, n, soft, ss, bits, bs, None)
    assert lib.srcdsp_sdpsk_step_batched(None, 1, DUMMY, 8, None, 8, DUMMY2, 8, None, 0, None) == capi.ERR_ARG
    assert lib.srcdsp_sdpsk_step_batched((C.c_void_p * 1)(a.h.value), 0, DUMMY, 8, None, 8, DUMMY2, 8, None, 0,
                                         None) == capi.ERR_ARG
    assert bank([a, None]) == capi.ERR_ARG and b"null handle" in lib.srcdsp_last_error()
    assert bank([a, b, a]) == capi.ERR_ARG and b"listed once" in lib.srcdsp_last_error()
    assert bank([a, c]) == capi.ERR_ARG and b"share D" in lib.srcdsp_last_error()
    assert lib.srcdsp_sdpsk_set_shift(b.h, 6) == 0
    assert bank([a, b]) == capi.ERR_ARG and b"share D" in lib.srcdsp_last_error()  # mixed shifts
    assert lib.srcdsp_sdpsk_set_shift(b.h, 5) == 0
    assert bank([a, b], d_in=None) == capi.ERR_ARG
    assert bank([a, b], soft=None) == capi.ERR_ARG and b"null buffer" in lib.srcdsp_last_error()
    assert bank([a, b], ss=7) == capi.ERR_SIZE
    assert bank([a, b], bits=DUMMY2, bs=7) == capi.ERR_SIZE and b"stride" in lib.srcdsp_last_error()
    assert bank([a, b], soft=None, ss=0, bits=DUMMY2, bs=7) == capi.ERR_SIZE
    # the rules hold when there is nothing to do, too; then n == 0 is fine
    assert bank([a, a], n=0) == capi.ERR_ARG
    assert bank([a, c], n=0) == capi.ERR_ARG
    assert bank([a, b], n=0, d_in=None, soft=None, ss=0) == capi.OK
    for x, st in zip((a, b, c), before):
        now = x.state()
        assert now[:2] == st[:2] and np.array_equal(now[2], st[2])


@pytest.mark.parametrize("D", DS)
def test_step_host_equals_the_model(capi, D):
    for n in (0, 1, D - 1, D, D + 1, 4099):
        for shift in (0, 17, 31):
            x = samples(n, 1000 * D + n)
            h, m = Handle(capi, D, shift), SdpskModel(D, shift)
            m.carry = samples(D, 7 * D + n)  # a carry that is not zero: step it in first
            h.step(m.carry)
            soft, bits = h.step(x)
            ms, mb = m.step(x)
            assert np.array_equal(soft, ms) and np.array_equal(bits, mb), (n, shift)
            d, s, carry = h.state()
            assert (d, s) == (D, shift) and np.array_equal(carry, m.carry), (n, shift)


def test_step_host_extremes_and_single_outputs(capi):
    """The two extreme pairs; soft alone and bits alone leave the other buffer."""
    for (a, b), soft, bit in zip(EXTREME, (127, -128), (1, 0)):
        for shift, want in ((0, soft), (24, soft), (31, 0 if bit else -1)):
            h = Handle(capi, 1, shift)
            h.step([b])
            s, bt = h.step([a])
            assert s[0] == want and bt[0] == bit
    x = samples(100, 5)
    m = SdpskModel(3, 12)
    ms, mb = m.step(x)
    h = Handle(capi, 3, 12)
    s, b = h.step(x, bits=False)
    assert np.array_equal(s, ms) and (b == 77).all()
    h = Handle(capi, 3, 12)
    s, b = h.step(x, soft=False)
    assert np.array_equal(b, mb) and (s == 77).all()


@pytest.mark.parametrize("D", DS)
def test_step_host_stream_in_unequal_chunks(capi, D):
    """The carry crosses calls, also calls shorter than D."""
    x = samples(3 * 64 + 200, 50 + D)
    whole_s, whole_b = SdpskModel(D, 9).step(x)
    h, m = Handle(capi, D, 9), SdpskModel(D, 9)
    cuts = [0, 1, 1 + max(D - 1, 0), 1 + max(D - 1, 0), 2 * D + 1, 2 * D + 3, 150, len(x)]
    got_s, got_b = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s, b = h.step(x[lo:hi])
        m.step(x[lo:hi])
        got_s.append(s)
        got_b.append(b)
        assert np.array_equal(h.state()[2], m.carry), (lo, hi)
    assert np.array_equal(np.concatenate(got_s), whole_s) and np.array_equal(np.concatenate(got_b), whole_b)


def test_reset_clone_and_set_shift(capi):
    x = samples(300, 9)
    h = Handle(capi, 5, 3)
    first = h.step(x[:100])
    c = h.clone()  # D, the shift and the carry
    assert c.state()[:2] == (5, 3) and np.array_equal(c.state()[2], x[95:100])
    a, b = h.step(x[100:]), c.step(x[100:])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], SdpskModel(5, 3, x[95:100]).step(x[100:])[0])
    h.reset()  # the carry is zero again, D and the shift stay
    assert h.state()[:2] == (5, 3) and not h.state()[2].any()
    again = h.step(x[:100])
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    assert np.array_equal(c.state()[2], x[-5:])  # the clone is its own object
    assert h.lib.srcdsp_sdpsk_set_shift(h.h, 11) == 0
    assert h.state()[:2] == (5, 11) and np.array_equal(h.state()[2], x[95:100])
    assert np.array_equal(h.step(x[100:])[0], SdpskModel(5, 11, x[95:100]).step(x[100:])[0])


def test_python_face_on_host_arrays():
    import srcdsp_amd as S
    x = samples(500, 11)
    d = S.DemodulatorSdpsk(D=2, shift=15)
    m = SdpskModel(2, 15)
    for lo, hi in ((0, 1), (1, 300), (300, 500)):
        soft, bits = d.step(x[lo:hi])
        ms, mb = m.step(x[lo:hi])
        assert soft.dtype == np.int8 and bits.dtype == np.uint8
        assert np.array_equal(soft, ms) and np.array_equal(bits, mb)
    D, shift, carry = d.state()
    assert (D, shift) == (2, 15) and np.array_equal(carry, m.carry)
    import copy
    e = copy.copy(d)
    d.reset()
    assert not d.state()[2].any() and np.array_equal(e.state()[2], m.carry)
    d.setShift(3)
    assert d.state()[1] == 3
    with pytest.raises(S.SrcdspError):
        S.DemodulatorSdpsk(D=65)
    # bits out feed the mapper unchanged
    bits = np.random.default_rng(3).integers(0, 2, 64).astype(np.uint8)
    sym = S.SymbolMapperSdpsk().step(bits)
    assert np.array_equal(S.DemodulatorSdpsk().step(sym)[1][1:], bits[1:])


# ------------------------------------------------- the arithmetic under sanitisers
@pytest.fixture(scope="module")
def sdpsk_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("sdpsk_host")
    exe = str(d / "sdpsk_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sdpsk_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.parametrize("D", DS)
def test_kernel_arithmetic_on_the_host_equals_the_model(sdpsk_host, D):
    """sdpsk_kernels.h compiled for the host under the address and
    undefined-behaviour sanitisers, on exactly sized buffers: soft bits, bits
    and the carry byte for byte, the extreme products included (no signed
    overflow)."""
    d, exe = sdpsk_host
    for chunks, shift in (((0,), 0), ((1,), 31), ((max(D - 1, 0), D, D + 1), 17), ((4099,), 0),
                          ((5, 0, max(D - 1, 0), 1, 700), 24)):
        n = sum(chunks)
        x = samples(n, 30 * D + n)
        carry = samples(D, 31 * D + n)
        if n >= 4 * D + 4:  # the extreme pairs, D apart
            for k, (a, b) in enumerate(EXTREME):
                x[D * (2 * k + 1) + 1], x[D * (2 * k) + 1] = a, b
        (d / "in.bin").write_bytes(carry.tobytes() + x.tobytes())
        # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
        r = subprocess.run([exe, "in.bin", "out.bin", str(D), str(shift), *[str(c) for c in chunks]], cwd=str(d),
                           capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0 and not r.stderr.strip(), (chunks, shift, r.returncode, r.stderr)
        m = SdpskModel(D, shift, carry)
        soft, bits = m.step(x)
        if n >= 4 * D + 4 and shift == 0:
            assert soft[D + 1] == 127 and bits[D + 1] == 1
        assert (d / "out.bin").read_bytes() == soft.tobytes() + bits.tobytes() + m.carry.tobytes(), (chunks, shift)


# ------------------------------------------------------------------ the drop-in
def test_dropin_class_over_the_c_abi(capi, tmp_path):
    """dsptl::DemodulatorSdpsk<int16_t> (include/srcdsp/demodulators.h) through
    tests/cpp/sdpsk_main.cpp: host vectors, both step overloads, copy, reset
    and setShift."""
    exe = str(tmp_path / "sdpsk_main")
    libdir = os.path.dirname(capi.LIB_PATH)
    x = samples(333, 13)
    (tmp_path / "in.bin").write_bytes(x.tobytes())
    for std, extra in (("gnu++11", []), ("c++14", ["-DNDEBUG"])):
        r = subprocess.run(["g++", f"-std={std}", "-O1", "-Wall", *extra, "-I", os.path.join(ROOT, "include", "srcdsp"),
                            os.path.join(ROOT, "tests", "cpp", "sdpsk_main.cpp"), "-L", libdir, "-lsrcdsp_hip",
                            f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for D, shift, cut in ((1, 0, 100), (4, 18, 2), (64, 31, 333)):
            r = subprocess.run([exe, "in.bin", "out.bin", str(D), str(shift), str(cut)], cwd=str(tmp_path),
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.returncode, r.stderr)
            soft, bits = SdpskModel(D, shift).step(x)
            assert (tmp_path / "out.bin").read_bytes() == soft.tobytes() + bits.tobytes(), (std, D, shift, cut)


# ---------------------------------------------------------------- the resources
def test_new_kernel_uses_no_scratch():
    """sdpsk_rows: the tile and its halo in LDS, no scratch."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "sdpsk.hip"), "sdpsk_rows", "400"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = []
    for ln in (ln for ln in r.stdout.splitlines() if "sdpsk_rows" in ln):
        f = ln[ln.rindex(" VGPR "):].split()
        rows.append({k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")})
    assert len(rows) == 1, r.stdout
    t = C.c_int()
    from srcdsp_amd import _capi
    assert _capi.lib().srcdsp_sdpsk_geometry(C.byref(t), None, None) == 0
    assert rows[0]["scratch"] == 0 and rows[0]["LDS"] == 4 * (t.value + 64 + 4) and rows[0]["VGPR"] <= 64, rows
