"""CPU-side checks of the batched correlator entry points
(srcdsp_corr_step_batched, srcdsp_corr_batched_stats): exported, in the ctypes
signature table, the argument rules that must refuse a call before any HIP
call, and the bank kernel's registers beside the single-channel scan's -- no
GPU here."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_corr_step_batched", "srcdsp_corr_batched_stats")


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_batched_correlator_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert hasattr(lib, s), s


def test_signature_table_covers_the_batched_correlator_symbols(capi):
    for s in NEW:
        assert s in capi.SIGNATURES, s
    res, args = capi.SIGNATURES["srcdsp_corr_step_batched"]
    assert res is C.c_int and len(args) == 8
    res, args = capi.SIGNATURES["srcdsp_corr_batched_stats"]
    assert res is C.c_int and len(args) == 2


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("corr_step_batched", "corr_batched_stats"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name


def test_null_arrays_are_an_argument_error(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    res = (C.c_int * 1)()
    for hs, found, idx in ((None, res, res), (one, None, res), (one, res, None), (None, None, None), (one, res, res)):
        rc = lib.srcdsp_corr_step_batched(hs, 1, None, 0, 0, found, idx, None)
        assert rc == capi.ERR_ARG, (hs, found, idx)
        assert lib.srcdsp_last_error()


def test_zero_channels_is_an_argument_error(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    res = (C.c_int * 1)()
    for ch in (0, -3):
        assert lib.srcdsp_corr_step_batched(one, ch, None, 0, 0, res, res, None) == capi.ERR_ARG


def _rows(src, name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", src), name],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if name + "(" in ln]
    assert len(rows) == 1, r.stdout + r.stderr[-2000:]
    f = rows[0]
    return {k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch")}


def test_bank_kernel_uses_no_scratch_and_no_more_registers_than_the_scan():
    """The gfx950 cross-compile of both users of the shared tile
    (corr_scan_kernels.h): no scratch in either, and the bank kernel within
    the single-channel scan's registers (its occupancy is tuned)."""
    scan, bank = _rows("corr.hip", "corr_scan_s1"), _rows("corr_bank.hip", "corr_bank_s1")
    assert scan["scratch"] == 0 and bank["scratch"] == 0, (scan, bank)
    assert bank["VGPR"] <= scan["VGPR"], (scan, bank)


def test_stats_are_zero_in_a_fresh_process(capi):
    code = ("from srcdsp_amd import _capi as A; import ctypes as C; b, l = C.c_ulong(7), C.c_ulong(7); "
            "assert A.lib().srcdsp_corr_batched_stats(C.byref(b), C.byref(l)) == 0; print(b.value, l.value)")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "0"]
