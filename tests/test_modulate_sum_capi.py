"""CPU-side checks of the summing modulator bank (srcdsp_modulate_sum_*):
exported, in the ctypes signature table and the header, marked as an extension
with the reference calls it composes; the argument rules that refuse a call
before any HIP call with every handle's state unchanged; the routing threshold
can be read and set; the kernel's gfx950 resources -- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mapper_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_modulate_sum_step", "srcdsp_modulate_sum_stats", "srcdsp_modulate_sum_geometry",
       "srcdsp_modulate_sum_set_min_tiles")
DUMMY = C.c_void_p(4096)    # never dereferenced: every call it goes to is refused
DUMMY2 = C.c_void_p(1 << 20)


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def test_library_exports_the_new_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_modulate_sum_step"][1]) == 13
    assert len(capi.SIGNATURES["srcdsp_modulate_sum_stats"][1]) == 2


def test_header_marks_the_extension_and_cites_what_it_composes(capi):
    with open(capi.HEADER) as f:
        text = f.read()
    at = text.index("SRCDSP_API int srcdsp_modulate_sum_step(")
    start = text.rindex("/*", 0, at)
    assert text.rindex("*/", 0, at) > start and not text[text.rindex("*/", 0, at) + 2:at].strip()
    doc = text[start:at]
    assert doc.startswith("/* Extension.")
    for cite in ("modulators.h:103-117 / :169-184", "upsampling_filters.h:149-233", "mixers.h:169-188",
                 "dsp_complex.h:83-108", "srcdsp_modulate_offset_step_batched", "srcdsp_modulate_step_batched",
                 "srcdsp_combine_step"):
        assert cite in doc, cite
    # which L the fused kernel serves and which it does not is said where the caller reads it
    assert "L = 2, 4 and 8" in doc and "L = 3, 5, 6 and 7" in doc and "no call at L = 4 or L = 8" in doc
    sec = text[at:text.index("FixedPatternCorrelator<int16_t, int32_t, N, S>")]
    assert sec.count("Extension") >= 3  # stats, geometry, set_min_tiles


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("modulate_sum_step", "modulate_sum_stats", "modulate_sum_geometry", "modulate_sum_set_min_tiles"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name


def _stats(lib):
    v = [C.c_ulong(7) for _ in range(2)]
    assert lib.srcdsp_modulate_sum_stats(*[C.byref(x) for x in v]) == 0
    return [x.value for x in v]


def test_stats_skip_null_pointers(capi):
    lib = capi.lib()
    assert lib.srcdsp_modulate_sum_stats(None, None) == capi.OK
    assert _stats(lib) == _stats(lib)


def test_geometry_and_threshold(capi):
    lib = capi.lib()

    def geometry(L):
        t, m, c = C.c_int(), C.c_long(-1), C.c_int(-1)
        assert lib.srcdsp_modulate_sum_geometry(L, C.byref(t), C.byref(m), C.byref(c)) == capi.OK
        assert t.value == 2048
        return m.value, c.value

    measured = {L: geometry(L) for L in range(1, 10)}
    # the measured routing, as the header and DESIGN 5.8c state it
    assert measured[2] == (2048, 8)
    assert all(measured[L] == (0, 0) for L in (1, 3, 4, 5, 6, 7, 8, 9))
    assert lib.srcdsp_modulate_sum_geometry(4, None, None, None) == capi.OK
    assert lib.srcdsp_modulate_sum_set_min_tiles(-1) == capi.ERR_ARG
    try:
        assert lib.srcdsp_modulate_sum_set_min_tiles(3) == capi.OK
        # every L the kernel exists for, up to kMaxBatch chains
        assert {L: geometry(L) for L in range(1, 10)} == {L: (3, 64) if L in (2, 4, 8) else (0, 0) for L in range(1, 10)}
    finally:
        assert lib.srcdsp_modulate_sum_set_min_tiles(0) == capi.OK
    assert {L: geometry(L) for L in range(1, 10)} == measured


def test_refusals_that_need_no_device_change_nothing(capi):
    """The rules that need no interpolator or mixer (those are device objects
    from their creation; tests/test_gpu_modulate_sum.py has the rest)."""
    lib = capi.lib()
    step = lib.srcdsp_modulate_sum_step
    before = _stats(lib)
    mp, mp2, g = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.srcdsp_mapper_create(C.byref(mp), M.QPSK) == 0 and lib.srcdsp_mapper_set_state(mp, 2) == 0
    assert lib.srcdsp_mapper_create(C.byref(mp2), M.QPSK) == 0
    assert lib.srcdsp_stagger_create(C.byref(g), 4) == 0
    x = np.arange(14, dtype=np.int16).reshape(-1, 2)
    y = np.zeros_like(x)
    assert lib.srcdsp_stagger_step_host(g, x.ctypes.data, len(x), y.ctypes.data) == 0  # a carry that is not zeros

    def carry():
        c = np.zeros(4, np.int16)
        assert lib.srcdsp_stagger_get_state(g, None, c.ctypes.data_as(C.POINTER(C.c_int16))) == 0
        return c.tolist()

    c0 = carry()
    assert any(c0)
    one_m, one_g = (C.c_void_p * 1)(mp.value), (C.c_void_p * 1)(g.value)
    none, fake = (C.c_void_p * 1)(None), (C.c_void_p * 1)(4096)
    args = (1, DUMMY, 0, DUMMY2, 64, 8, 0, 0, None)  # channels .. stream
    assert step(None, fake, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, None, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, one_g, None, *args) == capi.ERR_ARG
    assert b"no handles" in lib.srcdsp_last_error()
    for ch in (0, -2):
        assert step(one_m, fake, one_g, fake, ch, *args[1:]) == capi.ERR_ARG
    for shift in (16, 1 << 20):
        assert step(one_m, fake, one_g, fake, *args[:7], shift, None) == capi.ERR_ARG
        assert b"shift is 0..15" in lib.srcdsp_last_error()
    assert step(none, fake, one_g, fake, *args) == capi.ERR_ARG
    assert lib.srcdsp_last_error() == b"modulate_sum_step: null handle"
    assert step(one_m, none, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, none, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, one_g, none, *args) == capi.ERR_ARG
    assert step(one_m, none, None, fake, *args) == capi.ERR_ARG  # staggers may be NULL; the other lists are checked
    two_m, fake2 = (C.c_void_p * 2)(mp.value, mp2.value), (C.c_void_p * 2)(4096, 8192)
    for lists in (((C.c_void_p * 2)(mp.value, mp.value), fake2, (C.c_void_p * 2)(g.value, 12288), fake2),
                  (two_m, (C.c_void_p * 2)(4096, 4096), None, fake2),
                  (two_m, fake2, (C.c_void_p * 2)(g.value, g.value), fake2),
                  (two_m, fake2, None, (C.c_void_p * 2)(8192, 8192))):
        assert step(*lists, 2, *args[1:]) == capi.ERR_ARG  # a handle listed twice
        assert b"once" in lib.srcdsp_last_error()
    assert _stats(lib) == before  # nothing above ran
    assert carry() == c0
    k, s = C.c_int(), C.c_int()
    assert lib.srcdsp_mapper_get_state(mp, C.byref(k), C.byref(s)) == 0 and s.value == 2
    assert lib.srcdsp_stagger_destroy(g) == capi.OK
    assert lib.srcdsp_mapper_destroy(mp) == capi.OK and lib.srcdsp_mapper_destroy(mp2) == capi.OK


def test_python_face_refuses_mismatched_lists():
    import srcdsp_amd as S
    with pytest.raises(ValueError):
        S.modulate_sum_step([], [], None, [], None)
    with pytest.raises(ValueError):
        S.modulate_sum_step([S.SymbolMapperQpsk()], [], None, [], None)


def test_new_kernel_uses_no_scratch():
    """modsum_tile_dot2 for L in {2, 4, 8} x {8, 16 and 32 (L < 8) pairs compiled in,
    run-time taps} x {stagger, none}: the 2 * 8 L sums of a lane are registers,
    nothing spills to scratch."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", "modulate_sum.hip"), "modsum_tile_dot2", "400"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if "modsum_tile_dot2" in ln]
    assert len(rows) == 20, rows
    for ln in rows:
        f = ln[ln.rindex(" VGPR "):].split()
        assert int(f[f.index("scratch") + 1]) == 0, ln
