"""CPU-side checks of the DDC bank entry points (srcdsp_mixdecim_step_batched,
srcdsp_mixdecim_batched_stats): exported, in the ctypes signature table, and
the argument rules that must refuse a call before any HIP call -- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_mixdecim_step_batched", "srcdsp_mixdecim_batched_stats")


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_bank_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert hasattr(lib, s), s


def test_signature_table_covers_the_bank_symbols(capi):
    for s in NEW:
        assert s in capi.SIGNATURES, s
    res, args = capi.SIGNATURES["srcdsp_mixdecim_step_batched"]
    assert res is C.c_int and len(args) == 9
    res, args = capi.SIGNATURES["srcdsp_mixdecim_batched_stats"]
    assert res is C.c_int and len(args) == 2


def test_null_handle_arrays_are_an_argument_error(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    for hm, hd in ((None, None), (None, one), (one, None), (one, one)):
        rc = lib.srcdsp_mixdecim_step_batched(hm, hd, 1, None, 0, None, 0, 0, None)
        assert rc == capi.ERR_ARG, (hm, hd)
        assert lib.srcdsp_last_error()


def test_zero_channels_is_an_argument_error(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    for ch in (0, -3):
        assert lib.srcdsp_mixdecim_step_batched(one, one, ch, None, 0, None, 0, 0, None) == capi.ERR_ARG


def test_bank_kernel_uses_no_scratch():
    """The gfx950 cross-compile of the bank kernel: no scratch, and registers
    within the 128 of four waves per SIMD (its LDS allows four workgroups)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "ddc_bank.hip"), "ddc_bank_ci16"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if "ddc_bank_ci16" in ln]
    assert len(rows) == 1, r.stdout + r.stderr[-2000:]
    f = rows[0]
    assert int(f[f.index("scratch") + 1]) == 0, r.stdout
    assert int(f[f.index("VGPR") + 1]) <= 128, r.stdout


def test_stats_are_zero_in_a_fresh_process(capi):
    code = ("from srcdsp_amd import _capi as A; import ctypes as C; b, l = C.c_ulong(7), C.c_ulong(7); "
            "assert A.lib().srcdsp_mixdecim_batched_stats(C.byref(b), C.byref(l)) == 0; print(b.value, l.value)")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "0"]
