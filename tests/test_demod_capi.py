"""CPU-side checks of the demodulator entry points (srcdsp_demod_*): exported,
in the ctypes signature table, the argument rules that refuse a call before
any HIP call, the handle's host-side behaviour (a handle is a host object
until it steps), the kernel's per-sample arithmetic run on the host against
the goldens, and the kernel's gfx950 resources -- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import demod_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_demod_create", "srcdsp_demod_destroy", "srcdsp_demod_clone", "srcdsp_demod_set_sync_pattern",
       "srcdsp_demod_set_reference", "srcdsp_demod_set_reference_corr", "srcdsp_demod_set_initial_frequency",
       "srcdsp_demod_set_initial_phase", "srcdsp_demod_set_input_shift", "srcdsp_demod_reset",
       "srcdsp_demod_get_measured_frequency", "srcdsp_demod_get_state", "srcdsp_demod_get_tables",
       "srcdsp_demod_step", "srcdsp_demod_step_host", "srcdsp_demod_step_batched")
LDS_BYTES = 71424  # 48 KiB tables + 16 640 input tile + 4 352 soft tile + 1 280 row words
MAN, ARR = M.load_golden()


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_demodulator_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_demod_step_batched"][1]) == 11
    assert len(capi.SIGNATURES["srcdsp_demod_step"][1]) == 8


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("DemodulatorOqpsk", "demod_step_batched"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name


def test_null_handles_are_refused(capi):
    lib = capi.lib()
    ns, err, f = C.c_size_t(), C.c_int32(), C.c_float()
    assert lib.srcdsp_demod_create(None) == capi.ERR_ARG
    assert lib.srcdsp_demod_clone(None, None) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_sync_pattern(None, None, 0) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_reference(None, None, 0) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_reference_corr(None, None, None) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_initial_frequency(None, 0.0) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_initial_phase(None, 0.0) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_input_shift(None, 0) == capi.ERR_ARG
    assert lib.srcdsp_demod_reset(None) == capi.ERR_ARG
    assert lib.srcdsp_demod_get_measured_frequency(None, C.byref(f)) == capi.ERR_ARG
    assert lib.srcdsp_demod_get_state(None, *([None] * 10)) == capi.ERR_ARG
    assert lib.srcdsp_demod_step(None, None, 4, None, 4, C.byref(ns), C.byref(err), None) == capi.ERR_ARG
    assert lib.srcdsp_demod_step_host(None, None, 4, None, 4, C.byref(ns), C.byref(err)) == capi.ERR_ARG
    assert lib.srcdsp_demod_destroy(None) == capi.OK
    assert lib.srcdsp_last_error()


def test_batched_argument_rules(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    ns, err = (C.c_size_t * 1)(), (C.c_int32 * 1)()
    for ch in (0, -3):
        assert lib.srcdsp_demod_step_batched(one, ch, None, 0, None, 8, None, 8, ns, err, None) == capi.ERR_ARG
    for hs, a, b in ((None, ns, err), (one, None, err), (one, ns, None), (one, ns, err)):  # the last: a null handle
        assert lib.srcdsp_demod_step_batched(hs, 1, None, 0, None, 8, None, 8, a, b, None) == capi.ERR_ARG


def _state(lib, h):
    bc = C.c_uint()
    v = [C.c_int() for _ in range(9)]
    assert lib.srcdsp_demod_get_state(h, C.byref(bc), *[C.byref(x) for x in v]) == 0
    return (bc.value,) + tuple(x.value for x in v)


def test_handle_configuration_and_refusals_without_a_device(capi):
    """create, set_*, reset, clone and the refusals of step make no HIP call."""
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.srcdsp_demod_create(C.byref(h)) == capi.OK
    f = C.c_float(7)
    assert lib.srcdsp_demod_get_measured_frequency(h, C.byref(f)) == 0 and f.value == 0.0
    assert _state(lib, h) == (0,) * 10
    # frequency words: +-4096 taken, beyond refused and the word kept
    for w in (0, 13, -13, 4096, -4096):
        assert lib.srcdsp_demod_set_initial_frequency(h, float(M.word_freq(w))) == capi.OK
        assert _state(lib, h)[7] == w
    for bad in (3.15, -3.15, 100.0, float("nan"), float("inf")):
        assert lib.srcdsp_demod_set_initial_frequency(h, C.c_float(bad)) == capi.ERR_ARG
        assert b"4096" in lib.srcdsp_last_error()
        assert _state(lib, h)[7] == -4096
    for s in (-1, 16):
        assert lib.srcdsp_demod_set_input_shift(h, s) == capi.ERR_ARG
    bits = np.array([1, 0, 1, 1, 0], np.int8)
    bp = bits.ctypes.data_as(C.POINTER(C.c_int8))
    assert lib.srcdsp_demod_set_sync_pattern(h, bp, 1) == capi.ERR_ARG
    two = np.array([1, 2], np.int8)
    assert lib.srcdsp_demod_set_sync_pattern(h, two.ctypes.data_as(C.POINTER(C.c_int8)), 2) == capi.ERR_ARG
    assert lib.srcdsp_demod_set_sync_pattern(h, bp, 5) == capi.OK
    assert lib.srcdsp_demod_set_input_shift(h, 3) == capi.OK
    assert _state(lib, h)[9] == 3 and _state(lib, h)[3:5] == (0, 0)
    # reset (demodulators.cpp:293-308): the shift back to 0, bit1 / bit2 from the last two sync bits
    assert lib.srcdsp_demod_reset(h) == capi.OK
    st = _state(lib, h)
    assert st[9] == 0 and st[3:5] == (2 * 0 - 1, 2 * 1 - 1) and st[0] == 0
    m = M.DemodModel()
    m.set_sync_pattern(bits)
    m.set_initial_frequency(M.word_freq(-4096))
    m.reset()
    assert st == m.state()
    # clone: a value copy
    c = C.c_void_p()
    assert lib.srcdsp_demod_clone(h, C.byref(c)) == capi.OK and _state(lib, c) == st
    # refusals of step, all before any device call: first call of n <= P,
    # a reference shorter than the preamble, cap too small, n past INT_MAX
    ns, err = C.c_size_t(77), C.c_int32(77)
    dummy = C.c_void_p(16)
    assert lib.srcdsp_demod_step(h, dummy, 5, dummy, 5, C.byref(ns), C.byref(err), None) == capi.ERR_SIZE
    assert lib.srcdsp_demod_step(h, dummy, 40, dummy, 40, C.byref(ns), C.byref(err), None) == capi.ERR_SIZE  # no reference
    ref = np.zeros((4, 2), np.int16)
    assert lib.srcdsp_demod_set_reference(h, ref.ctypes.data_as(capi.I16P), 4) == capi.OK
    assert lib.srcdsp_demod_step(h, dummy, 40, dummy, 34, C.byref(ns), C.byref(err), None) == capi.ERR_SIZE  # cap < 35
    assert lib.srcdsp_demod_step(h, dummy, 1 << 31, dummy, 1 << 31, C.byref(ns), C.byref(err), None) == capi.ERR_SIZE
    hs = (C.c_void_p * 2)(h.value, h.value)
    ns2, err2 = (C.c_size_t * 2)(), (C.c_int32 * 2)()
    assert lib.srcdsp_demod_step_batched(hs, 2, dummy, 0, None, 40, dummy, 40, ns2, err2, None) == capi.ERR_ARG  # twice
    assert (ns.value, err.value) == (77, 77) and _state(lib, h) == st
    # n = 0: OK, nothing changes
    assert lib.srcdsp_demod_step(h, None, 0, None, 0, C.byref(ns), C.byref(err), None) == capi.OK
    assert ns.value == 0 and _state(lib, h) == st
    assert lib.srcdsp_demod_destroy(h) == capi.OK and lib.srcdsp_demod_destroy(c) == capi.OK


def test_library_tables_equal_the_reference_tables(capi):
    """Built on this host with the reference's expressions; the GPU suite asks
    the same of the GPU box's libm (tests/test_gpu_demod.py)."""
    from srcdsp_amd import demod_tables
    s, p = demod_tables()
    assert np.array_equal(s, ARR["sine"]) and np.array_equal(p, ARR["phase"])


@pytest.fixture(scope="module")
def lane_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("demod_lane")
    exe = str(d / "demod_lane_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "demod_lane_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.concatenate([ARR["sine"], ARR["phase"]]).astype(np.int16).tofile(str(d / "tables.bin"))
    return d, exe


@pytest.mark.parametrize("key", [c["key"] for c in MAN["cases"]])
def test_kernel_arithmetic_on_the_host_equals_the_reference(lane_host, key):
    """demod_sample (demod_kernels.h), the one source of the kernel's
    per-sample arithmetic, compiled for the host under the address and
    undefined-behaviour sanitisers: every golden case byte for byte."""
    d, exe = lane_host
    (d / "case.bin").write_bytes(ARR[key + "_case"].tobytes())
    # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
    r = subprocess.run([exe, "case.bin", "tables.bin", "out.bin"], cwd=str(d), capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    assert (d / "out.bin").read_bytes() == ARR[key + "_out"].tobytes()


def test_quick_phase_halving_closed_form_equals_the_loop():
    """demod_quick_phase replaces the reference's halving loop by a ceiling
    division by 2^k; both restated here and compared over every pair of
    magnitudes that decides a distinct k."""
    def loop(re, im):
        while re >= 128 or im >= 128:
            re, im = (re + 1) // 2, (im + 1) // 2
        return re, im

    def closed(re, im):
        m = max(re, im)
        k = 0 if m < 128 else m.bit_length() - 7
        if (m + (1 << k) - 1) >> k >= 128:
            k += 1
        return (re + (1 << k) - 1) >> k, (im + (1 << k) - 1) >> k

    edge = sorted({v for b in range(7, 16) for v in ((1 << b) - 2, (1 << b) - 1, 1 << b, (1 << b) + 1,
                                                      127 << (b - 7), (127 << (b - 7)) + 1)} | {0, 1, 126, 32767})
    edge = [v for v in edge if 0 <= v <= 32767]
    rng = np.random.default_rng(5)
    vals = edge + rng.integers(0, 32768, 300).tolist()
    for re in vals:
        for im in edge:
            assert loop(re, im) == closed(re, im), (re, im)


def _rows(name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "demod.hip"), name],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if name + "(" in ln]
    assert len(rows) == 1, r.stdout + r.stderr[-2000:]
    f = rows[0]
    return {k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")}


def test_bank_kernel_uses_no_scratch_and_the_lds_design_quotes():
    row = _rows("demod_bank")
    assert row["scratch"] == 0, row
    assert row["LDS"] == LDS_BYTES, row
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "71 424" in f.read()
    assert MAN["tile"] == 64  # kDemodTile
