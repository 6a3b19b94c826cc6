"""CPU-side checks of the frequency estimator entry points (srcdsp_freqest_*,
srcdsp_demod_acquire_batched): exported, in the ctypes signature table, the
argument rules that refuse or answer a call before any HIP call, the library's
per-pair arithmetic run on the host against the goldens, and the kernels'
gfx950 resources -- no GPU here.

A correlator handle cannot be made without a device (srcdsp_corr_create
allocates its device buffers), so of the join only the refusals that need no
handle are here; `first` out of range, a word outside +-4096, a demodulator
taken twice and the join's results are in tests/test_gpu_acquire_chain.py."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import freqest_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_freqest_create", "srcdsp_freqest_destroy", "srcdsp_freqest_geometry", "srcdsp_freqest_run",
       "srcdsp_freqest_run_host", "srcdsp_freqest_run_batched", "srcdsp_demod_acquire_batched")
MAN, ARR = M.load_golden()


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_estimator_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_freqest_run"][1]) == 7
    assert len(capi.SIGNATURES["srcdsp_freqest_run_host"][1]) == 6
    assert len(capi.SIGNATURES["srcdsp_freqest_run_batched"][1]) == 10
    assert len(capi.SIGNATURES["srcdsp_demod_acquire_batched"][1]) == 8
    with open(capi.HEADER) as f:
        assert "dsptl_miscellaneous.h:43-58" in f.read()


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("FreqEstimator", "estimate_freq", "demod_acquire_batched"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name
    with pytest.raises(TypeError):
        srcdsp_amd.FreqEstimator(1, InType="float")


def _handle(lib, L):
    h = C.c_void_p()
    assert lib.srcdsp_freqest_create(C.byref(h), L) == 0
    return h


def test_refusals_and_empty_answers_before_any_hip_call(capi):
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.srcdsp_freqest_create(None, 1) == capi.ERR_ARG
    for L in (0, -1):
        assert lib.srcdsp_freqest_create(C.byref(h), L) == capi.ERR_ARG and not h.value
    assert lib.srcdsp_freqest_destroy(None) == capi.OK
    h = _handle(lib, 4)
    t, v, gl = C.c_int(), C.c_int(), C.c_int()
    assert lib.srcdsp_freqest_geometry(None, None, None, None, None) == capi.ERR_ARG
    assert lib.srcdsp_freqest_geometry(h, C.byref(gl), C.byref(t), C.byref(v), None) == capi.OK
    assert (gl.value, v.value) == (4, 4) and t.value % (64 * v.value) == 0
    f, s, e = C.c_float(7), (C.c_int64 * 2)(7, 7), C.c_int(7)
    dummy = C.c_void_p(16)
    # nulls
    assert lib.srcdsp_freqest_run(None, dummy, 100, C.byref(f), s, C.byref(e), None) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run(h, dummy, 100, None, s, C.byref(e), None) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run(h, None, 100, C.byref(f), s, C.byref(e), None) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run_host(None, dummy, 100, C.byref(f), s, C.byref(e)) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run_host(h, dummy, 100, None, s, C.byref(e)) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run_host(h, None, 100, C.byref(f), s, C.byref(e)) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run_batched(None, 1, dummy, 0, None, 100, C.byref(f), s, C.byref(e), None) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run_batched(h, 1, dummy, 0, None, 100, None, s, C.byref(e), None) == capi.ERR_ARG
    assert lib.srcdsp_freqest_run_batched(h, 1, None, 0, None, 100, C.byref(f), s, C.byref(e), None) == capi.ERR_ARG
    # channels < 1
    for ch in (0, -2):
        assert lib.srcdsp_freqest_run_batched(h, ch, dummy, 0, None, 100, C.byref(f), s, C.byref(e), None) == capi.ERR_ARG
    # n past INT_MAX
    big = 1 << 31
    assert lib.srcdsp_freqest_run(h, dummy, big, C.byref(f), s, C.byref(e), None) == capi.ERR_SIZE
    assert lib.srcdsp_freqest_run_host(h, dummy, big, C.byref(f), s, C.byref(e)) == capi.ERR_SIZE
    assert lib.srcdsp_freqest_run_batched(h, 1, dummy, 0, None, big, C.byref(f), s, C.byref(e), None) == capi.ERR_SIZE
    assert lib.srcdsp_last_error()
    assert (f.value, s[0], s[1], e.value) == (7.0, 7, 7, 7)  # a refused call writes nothing
    # n = 0 and n <= L: OK, +0.0f, zero sums, exact; the buffer is not looked at
    for n in (0, 1, 4):
        for call in (lambda: lib.srcdsp_freqest_run(h, None, n, C.byref(f), s, C.byref(e), None),
                     lambda: lib.srcdsp_freqest_run_host(h, None, n, C.byref(f), s, C.byref(e))):
            f.value, s[0], s[1], e.value = 7, 7, 7, 7
            assert call() == capi.OK
            assert M.bits(f.value) == 0 and (s[0], s[1], e.value) == (0, 0, 1)
    f3, s3, e3 = (C.c_float * 3)(7, 7, 7), (C.c_int64 * 6)(*([7] * 6)), (C.c_int * 3)(7, 7, 7)
    assert lib.srcdsp_freqest_run_batched(h, 3, None, 0, None, 4, f3, s3, e3, None) == capi.OK
    assert list(f3) == [0.0] * 3 and list(s3) == [0] * 6 and list(e3) == [1] * 3
    # sums and exact may be NULL
    assert lib.srcdsp_freqest_run(h, None, 3, C.byref(f), None, None, None) == capi.OK
    assert lib.srcdsp_freqest_run_batched(h, 3, None, 0, None, 4, f3, None, None, None) == capi.OK
    assert lib.srcdsp_freqest_destroy(h) == capi.OK


def test_join_refusals_that_need_no_handle(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    f = (C.c_float * 1)(7)
    assert lib.srcdsp_demod_acquire_batched(None, one, 1, None, 1, 1, -1.0, f) == capi.ERR_ARG
    assert lib.srcdsp_demod_acquire_batched(one, None, 1, None, 1, 1, -1.0, f) == capi.ERR_ARG
    for ch in (0, -1):
        assert lib.srcdsp_demod_acquire_batched(one, one, ch, None, 1, 1, -1.0, f) == capi.ERR_ARG
    for L in (0, -5):
        assert lib.srcdsp_demod_acquire_batched(one, one, 1, None, L, 1, -1.0, f) == capi.ERR_ARG
    assert lib.srcdsp_demod_acquire_batched(one, one, 1, None, 1, 1, -1.0, f) == capi.ERR_ARG  # null handles, taken
    assert b"null handle" in lib.srcdsp_last_error()
    # a channel not taken is not looked at
    none = (C.c_int * 1)(0)
    assert lib.srcdsp_demod_acquire_batched(one, one, 1, none, 1, 1, -1.0, f) == capi.OK
    assert f[0] == 7.0


@pytest.fixture(scope="module")
def pair_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("freqest_host")
    exe = str(d / "freqest_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "freqest_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


def _run_host(pair_host, cases):
    """cases: [(L, x)] -> [(float bits, sumI, sumQ, exact)], one process."""
    d, exe = pair_host
    args = []
    for i, (L, x) in enumerate(cases):
        x = np.ascontiguousarray(x, np.int16).reshape(-1, 2)
        (d / f"{i}.case").write_bytes(struct.pack("<ii", L, len(x)) + x.tobytes())
        args += [f"{i}.case", f"{i}.out"]
    # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
    r = subprocess.run([exe] + args, cwd=str(d), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    return [struct.unpack("<Iqqi", (d / f"{i}.out").read_bytes()) for i in range(len(cases))]


def test_pair_arithmetic_on_the_host_equals_the_reference(pair_host):
    """freqest_pair (freqest_pair.h), the one source of the kernel's, the host
    form's and the join's arithmetic, compiled for the host under the address
    and undefined-behaviour sanitisers: every golden bit for bit."""
    cases = MAN["cases"]
    got = _run_host(pair_host, [(c["L"], ARR[c["input"]][:c["n"]]) for c in cases])
    for c, (b, si, sq, ex) in zip(cases, got):
        f, sums, exact = M.estimate(ARR[c["input"]][:c["n"]], c["L"])
        assert b == c["bits"] and (si, sq) == sums and ex == int(exact) == 1, c["key"]


def test_pair_arithmetic_wraps_at_the_corner_without_undefined_behaviour(pair_host):
    """x[i] = x[i+L] = (-32768, -32768): termI = 2^31 wraps to -2^31, taken in
    unsigned, so the sanitised build runs clean; |term| = 2^31 enters the bound."""
    rng = np.random.default_rng(7)
    cases = []
    for L in (1, 3):
        x = rng.integers(-32768, 32768, size=(500, 2)).astype(np.int16)
        x[100:140] = -32768
        x[300] = x[300 + L] = -32768
        cases.append((L, x))
        cases.append((L, np.full((L + 2, 2), -32768, np.int16)))
    cases.append((1, np.full(((1 << 22) + 2, 2), -32768, np.int16)))  # 2^22 + 1 pairs of 2^31: past the bound
    got = _run_host(pair_host, cases)
    for (L, x), (b, si, sq, ex) in zip(cases, got):
        f, sums, exact = M.estimate(x, L)
        assert b == M.bits(f) and (si, sq) == sums and ex == int(exact), (L, len(x))
    assert got[1][1] == -2 * (1 << 31) and got[-1][3] == 0


def _rows(name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "freqest.hip"), name],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if name + "(" in ln]
    assert len(rows) == 1, r.stdout + r.stderr[-2000:]
    f = rows[0]
    return {k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")}


@pytest.mark.parametrize("name", ["freqest_rows", "freqest_finish"])
def test_kernels_use_no_scratch(name):
    """freqest_rows serves the single row and the bank (the single row is the
    bank at one row); freqest_finish sums the slabs."""
    row = _rows(name)
    assert row["scratch"] == 0, row
