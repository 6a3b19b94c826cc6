"""CPU-side checks of the interpolator -> decimator entry points
(srcdsp_resample_step, srcdsp_resample_step_batched, srcdsp_resample_stats):
exported, in the ctypes signature table, the argument rules that must refuse a
call before any HIP call, the fused kernel's gfx950 resources and the tile's
index arithmetic (resample_index.h) replayed by a sanitized host program -- no
GPU here."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"srcdsp_resample_step": 8, "srcdsp_resample_step_batched": 10, "srcdsp_resample_stats": 4}
INSTANCES = {(2, 16), (4, 16), (8, 8)} | {(L, 0) for L in range(2, 9)}


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def geometry(capi):
    tile, cap = C.c_int(), C.c_int()
    assert capi.lib().srcdsp_resample_geometry(C.byref(tile), C.byref(cap)) == capi.OK
    return tile.value, cap.value


def test_library_exports_the_resample_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert hasattr(lib, s), s


def test_signature_table_covers_the_resample_symbols(capi):
    for s, arity in NEW.items():
        assert s in capi.SIGNATURES, s
        res, args = capi.SIGNATURES[s]
        assert res is C.c_int and len(args) == arity, s


def test_package_exports_the_python_layer():
    import srcdsp_amd
    for name in ("RationalResampler", "resample_step_batched", "resample_stats"):
        assert name in srcdsp_amd.__all__ and hasattr(srcdsp_amd, name), name


def test_null_handles_are_an_argument_error(capi):
    lib = capi.lib()
    assert lib.srcdsp_resample_step(None, None, None, 0, None, 0, 0, None) == capi.ERR_ARG
    assert lib.srcdsp_last_error()
    one = (C.c_void_p * 1)(None)
    for hu, hd in ((None, None), (None, one), (one, None), (one, one)):
        rc = lib.srcdsp_resample_step_batched(hu, hd, 1, None, 0, None, 0, 0, 0, None)
        assert rc == capi.ERR_ARG, (hu, hd)
        assert lib.srcdsp_last_error()


def test_zero_channels_is_an_argument_error(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    for ch in (0, -3):
        assert lib.srcdsp_resample_step_batched(one, one, ch, None, 0, None, 0, 0, 0, None) == capi.ERR_ARG


def test_stats_are_zero_in_a_fresh_process(capi):
    code = ("from srcdsp_amd import _capi as A; import ctypes as C; v = [C.c_ulong(7) for _ in range(4)]; "
            "assert A.lib().srcdsp_resample_stats(*[C.byref(x) for x in v]) == 0; print(*[x.value for x in v])")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "0", "0", "0"]


def test_fused_kernel_resources_are_the_ones_design_quotes():
    """The gfx950 cross-compile of every resample_tile_dot2 instantiation: no
    scratch and no static LDS; DESIGN.md quotes the registers of the measured
    L = 4 shape (16 tap pairs per phase compiled in)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "resample.hip"), "resample_tile_dot2", "256"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.search(r"resample_tile_dot2<(\d+), (\d+)>", ln)
        if m:
            f = ln.split()
            rows[(int(m.group(1)), int(m.group(2)))] = {k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")}
    assert set(rows) == INSTANCES, r.stdout + r.stderr[-2000:]
    for k, v in rows.items():
        assert v["scratch"] == 0 and v["LDS"] == 0, (k, v)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert f"resample_tile_dot2<4, 16>: {rows[(4, 16)]['VGPR']} VGPRs" in design, rows[(4, 16)]


def test_tile_index_arithmetic_under_host_sanitizers(capi, tmp_path):
    """tests/cpp/resample_index_main.cpp: a stand-alone program over
    resample_index.h, built with -fsanitize=address,undefined and run as a
    program.  It also prints the launcher's dynamic LDS at L = 8 with the
    decimator tap cap, which must fit the 160 KiB of a CU."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    tile, cap = geometry(capi)
    assert tile == 2048 and cap >= 256
    exe = str(tmp_path / "resample_index")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "resample_index_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(cap)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout
    lds = int(re.search(r"smem L=8 H=512 Nd=%d: (\d+)" % cap, r.stdout).group(1))
    assert lds <= 160 * 1024, lds
