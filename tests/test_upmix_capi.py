"""CPU-side checks of the interpolator -> mixer chain entry points
(srcdsp_upmix_step, srcdsp_upmix_step_batched, srcdsp_upmix_stats): exported,
in the ctypes signature table, the argument rules that must refuse a call
before any HIP call, the fused kernel's gfx950 resources, and the shape
dispatcher of the v_dot2 transmit tiles (up_dot2_dispatch.h) swept by a
sanitized host program -- no GPU here."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"srcdsp_upmix_step": 9, "srcdsp_upmix_step_batched": 10, "srcdsp_upmix_stats": 4}


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_upmix_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert hasattr(lib, s), s


def test_signature_table_covers_the_upmix_symbols(capi):
    for s, arity in NEW.items():
        assert s in capi.SIGNATURES, s
        res, args = capi.SIGNATURES[s]
        assert res is C.c_int and len(args) == arity, s


def test_package_exports_the_python_layer():
    import srcdsp_amd
    for name in ("UpsamplerMixerChain", "upmix_step_batched", "upmix_stats"):
        assert name in srcdsp_amd.__all__ and hasattr(srcdsp_amd, name), name


def test_null_handles_are_an_argument_error(capi):
    lib = capi.lib()
    assert lib.srcdsp_upmix_step(None, None, None, 0, None, 0, 0, 0, None) == capi.ERR_ARG
    assert lib.srcdsp_last_error()
    one = (C.c_void_p * 1)(None)
    for hu, hm in ((None, None), (None, one), (one, None), (one, one)):
        rc = lib.srcdsp_upmix_step_batched(hu, hm, 1, None, 0, None, 0, 0, 0, None)
        assert rc == capi.ERR_ARG, (hu, hm)
        assert lib.srcdsp_last_error()


def test_zero_channels_is_an_argument_error(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    for ch in (0, -3):
        assert lib.srcdsp_upmix_step_batched(one, one, ch, None, 0, None, 0, 0, 0, None) == capi.ERR_ARG


def test_fused_kernel_resources_are_the_ones_design_quotes():
    """The gfx950 cross-compile of every fused instantiation: no scratch and no
    static LDS.  At the measured shape (L = 4, 16 tap pairs per phase compiled
    in) and at L = 4 with run-time taps the registers stay within the 168 of
    three waves per SIMD -- the three workgroups per CU that 44 KiB of dynamic
    LDS (36 KiB tile + the 8 KiB table of N = 4096) allow -- and DESIGN.md
    quotes the very figures."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "upmix.hip"), "upmix_tile_dot2", "200"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.search(r"upmix_tile_dot2<(\d+), (\d+)>", ln)
        if m:
            f = ln.split()
            rows[(int(m.group(1)), int(m.group(2)))] = {k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")}
    assert len(rows) == 15, r.stdout + r.stderr[-2000:]
    for k, v in rows.items():
        assert v["scratch"] == 0 and v["LDS"] == 0, (k, v)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    for k in ((4, 16), (4, 0)):
        assert rows[k]["VGPR"] <= 168, (k, rows[k])
        assert f"upmix_tile_dot2<{k[0]}, {k[1]}>: {rows[k]['VGPR']} VGPRs" in design, (k, rows[k])
    tile_lds = max(4 * 16 * (256 + 4), 16 * 256 * (8 * 4 // 4 + 1))  # planes (16 pairs: 4 halo granules) / output tile
    assert tile_lds + 2 * 4096 == 45056 and "45 056" in design
    assert 3 * 45056 <= 160 * 1024 < 4 * 45056


def test_stats_are_zero_in_a_fresh_process(capi):
    code = ("from srcdsp_amd import _capi as A; import ctypes as C; v = [C.c_ulong(7) for _ in range(4)]; "
            "assert A.lib().srcdsp_upmix_stats(*[C.byref(x) for x in v]) == 0; print(*[x.value for x in v])")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "0", "0", "0"]


def test_tile_shape_dispatcher_under_host_sanitizers(tmp_path):
    """tests/cpp/up_dot2_dispatch_main.cpp: a stand-alone program over
    up_dot2_dispatch.h, built with -fsanitize=address,undefined and run as a
    program.  For the three families' shape tables, every L = 1..9 and PP =
    1..2048: one call of the callback where the family has the ratio, none
    otherwise, with the <LR, PPC> of a table written out a second time there;
    15, 10 and 10 kernels are reached (the summing tile's 10 twice, with and
    without staggers)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "up_dot2_dispatch")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "up_dot2_dispatch_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert re.search(r"^55296 cases, 0 failures$", r.stdout, re.M), r.stdout  # 3 families x 9 L x 2048 PP
    for family, n in (("standard", 15), ("resampler", 10), ("summing tile", 10)):
        assert f"{family}: {n} kernels" in r.stdout, r.stdout
