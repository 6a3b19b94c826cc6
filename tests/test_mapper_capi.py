"""CPU-side checks of the symbol mapper and modulator entry points
(srcdsp_mapper_*, srcdsp_modulate_*): exported, in the ctypes signature table
and the header, the argument rules that refuse a call before any HIP call with
the handle's state unchanged, the handle's host-side behaviour (a handle is a
host object until it steps on the device), the kernels' arithmetic run on the
host under sanitisers against the goldens, and the kernels' gfx950 resources
-- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mapper_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_mapper_create", "srcdsp_mapper_destroy", "srcdsp_mapper_clone", "srcdsp_mapper_reset",
       "srcdsp_mapper_get_state", "srcdsp_mapper_set_state", "srcdsp_mapper_geometry", "srcdsp_mapper_step",
       "srcdsp_mapper_step_host", "srcdsp_mapper_step_batched", "srcdsp_modulate_step",
       "srcdsp_modulate_step_batched", "srcdsp_modulate_stats")
MAN, ARR = M.load_golden()
DUMMY = C.c_void_p(4096)  # never dereferenced: every call below is refused, or has nothing to do


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def _new(lib, kind):
    h = C.c_void_p()
    assert lib.srcdsp_mapper_create(C.byref(h), kind) == 0
    return h


def _state(lib, h):
    k, s = C.c_int(-1), C.c_int(-1)
    assert lib.srcdsp_mapper_get_state(h, C.byref(k), C.byref(s)) == 0
    return k.value, s.value


def test_library_exports_the_new_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_mapper_step_batched"][1]) == 8
    assert len(capi.SIGNATURES["srcdsp_modulate_step"][1]) == 10
    assert len(capi.SIGNATURES["srcdsp_modulate_step_batched"][1]) == 11
    with open(capi.HEADER) as f:
        text = f.read()
    assert "#define SRCDSP_MAPPER_SDPSK 0" in text and "#define SRCDSP_MAPPER_QPSK 1" in text


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("SymbolMapperSdpsk", "SymbolMapperQpsk", "mapper_step_batched", "ModulatorChain",
                 "modulate_step_batched", "modulate_stats"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name


def test_geometry(capi):
    t = C.c_int()
    assert capi.lib().srcdsp_mapper_geometry(C.byref(t)) == 0
    assert t.value == 4096  # 256 lanes x one 16-byte load


def test_null_handles_and_unknown_kinds_are_refused(capi):
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.srcdsp_mapper_create(None, 0) == capi.ERR_ARG
    for kind in (-1, 2, 7):
        assert lib.srcdsp_mapper_create(C.byref(h), kind) == capi.ERR_ARG and not h.value
    assert lib.srcdsp_mapper_clone(None, C.byref(h)) == capi.ERR_ARG
    assert lib.srcdsp_mapper_reset(None) == capi.ERR_ARG
    assert lib.srcdsp_mapper_get_state(None, None, None) == capi.ERR_ARG
    assert lib.srcdsp_mapper_set_state(None, 0) == capi.ERR_ARG
    assert lib.srcdsp_mapper_step(None, DUMMY, 4, DUMMY, 4, None) == capi.ERR_ARG
    assert lib.srcdsp_mapper_step_host(None, DUMMY, 4, DUMMY, 4) == capi.ERR_ARG
    assert lib.srcdsp_modulate_step(None, None, None, DUMMY, 4, DUMMY, 16, 0, 0, None) == capi.ERR_ARG
    assert lib.srcdsp_mapper_destroy(None) == capi.OK
    assert lib.srcdsp_last_error()


def test_handle_lives_on_the_host_until_it_steps(capi):
    """create, reset, set_state, get_state and clone make no HIP call (this
    test runs where there is no device)."""
    lib = capi.lib()
    for kind in (M.SDPSK, M.QPSK):
        h = _new(lib, kind)
        assert _state(lib, h) == (kind, 0)
        for s in (3, 1, 2, 0, 2):
            assert lib.srcdsp_mapper_set_state(h, s) == capi.OK and _state(lib, h) == (kind, s)
        for bad in (-1, 4, 1 << 20):
            assert lib.srcdsp_mapper_set_state(h, bad) == capi.ERR_ARG and _state(lib, h) == (kind, 2)
        c = C.c_void_p()
        assert lib.srcdsp_mapper_clone(h, C.byref(c)) == capi.OK and _state(lib, c) == (kind, 2)
        assert lib.srcdsp_mapper_reset(h) == capi.OK and _state(lib, h) == (kind, 0)
        assert _state(lib, c) == (kind, 2)  # a value copy
        assert lib.srcdsp_mapper_destroy(h) == capi.OK and lib.srcdsp_mapper_destroy(c) == capi.OK


def test_step_refusals_change_nothing(capi):
    lib = capi.lib()
    s, q = _new(lib, M.SDPSK), _new(lib, M.QPSK)
    assert lib.srcdsp_mapper_set_state(s, 3) == 0 and lib.srcdsp_mapper_set_state(q, 1) == 0
    for fn, tail in ((lib.srcdsp_mapper_step, (None,)), (lib.srcdsp_mapper_step_host, ())):
        # wrong n_out for the kind, an odd QPSK bit count included
        for h, nb, no in ((s, 8, 7), (s, 8, 9), (s, 8, 4), (q, 8, 8), (q, 8, 3), (q, 7, 3), (q, 7, 4), (q, 1, 0)):
            assert fn(h, DUMMY, nb, DUMMY, no, *tail) == capi.ERR_SIZE, (nb, no)
        assert fn(s, None, 8, DUMMY, 8, *tail) == capi.ERR_ARG
        assert fn(s, DUMMY, 8, None, 8, *tail) == capi.ERR_ARG
        assert fn(q, None, 8, DUMMY, 4, *tail) == capi.ERR_ARG
        # no bits: OK, and nothing changes (null buffers are fine)
        assert fn(s, None, 0, None, 0, *tail) == capi.OK and fn(q, None, 0, None, 0, *tail) == capi.OK
    assert _state(lib, s) == (M.SDPSK, 3) and _state(lib, q) == (M.QPSK, 1)
    for h in (s, q):
        assert lib.srcdsp_mapper_destroy(h) == capi.OK


def test_batched_argument_rules(capi):
    lib = capi.lib()
    step = lib.srcdsp_mapper_step_batched
    s0, s1, q = _new(lib, M.SDPSK), _new(lib, M.SDPSK), _new(lib, M.QPSK)
    assert lib.srcdsp_mapper_set_state(s0, 1) == 0 and lib.srcdsp_mapper_set_state(s1, 2) == 0
    two = (C.c_void_p * 2)(s0.value, s1.value)
    for ch in (0, -3):
        assert step(two, ch, DUMMY, 0, DUMMY, 8, 8, None) == capi.ERR_ARG
    assert step(None, 2, DUMMY, 0, DUMMY, 8, 8, None) == capi.ERR_ARG
    assert step((C.c_void_p * 2)(s0.value, None), 2, DUMMY, 0, DUMMY, 8, 8, None) == capi.ERR_ARG
    assert step((C.c_void_p * 2)(s0.value, s0.value), 2, DUMMY, 0, DUMMY, 8, 8, None) == capi.ERR_ARG  # listed twice
    assert b"once" in lib.srcdsp_last_error()
    assert step((C.c_void_p * 2)(s0.value, q.value), 2, DUMMY, 0, DUMMY, 8, 8, None) == capi.ERR_ARG  # kinds differ
    assert step(two, 2, DUMMY, 7, DUMMY, 8, 8, None) == capi.ERR_ARG      # 0 < bits_stride < n_bits
    assert step(two, 2, DUMMY, 8, DUMMY, 7, 8, None) == capi.ERR_SIZE     # out_stride < symbols
    assert step(two, 2, None, 8, DUMMY, 8, 8, None) == capi.ERR_ARG
    assert step(two, 2, DUMMY, 8, None, 8, 8, None) == capi.ERR_ARG
    one_q = (C.c_void_p * 1)(q.value)
    assert step(one_q, 1, DUMMY, 0, DUMMY, 8, 7, None) == capi.ERR_SIZE   # odd QPSK bit count
    assert step(one_q, 1, DUMMY, 0, DUMMY, 3, 8, None) == capi.ERR_SIZE   # 4 symbols in a stride of 3
    assert step(two, 2, None, 0, None, 0, 0, None) == capi.OK             # no bits
    assert _state(lib, s0) == (M.SDPSK, 1) and _state(lib, s1) == (M.SDPSK, 2) and _state(lib, q) == (M.QPSK, 0)
    for h in (s0, s1, q):
        assert lib.srcdsp_mapper_destroy(h) == capi.OK


def test_modulate_batched_refuses_missing_and_repeated_handles(capi):
    """The rules that need no interpolator or mixer (those are device objects
    from their creation; tests/test_gpu_modulate.py has the rest)."""
    lib = capi.lib()
    step = lib.srcdsp_modulate_step_batched

    def stats():
        v = [C.c_ulong(7) for _ in range(4)]
        assert lib.srcdsp_modulate_stats(*[C.byref(x) for x in v]) == capi.OK
        return [x.value for x in v]

    before = stats()
    s0 = _new(lib, M.SDPSK)
    one = (C.c_void_p * 1)(s0.value)
    none = (C.c_void_p * 1)(None)
    fake = (C.c_void_p * 1)(4096)
    assert step(None, fake, fake, 1, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert step(one, None, fake, 1, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert step(one, fake, None, 1, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert step(one, fake, fake, 0, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert step(none, fake, fake, 1, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert step(one, none, fake, 1, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert step(one, fake, none, 1, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    twice = (C.c_void_p * 2)(s0.value, s0.value)
    fake2 = (C.c_void_p * 2)(4096, 8192)
    assert step(twice, fake2, fake2, 2, DUMMY, 0, DUMMY, 64, 8, 0, None) == capi.ERR_ARG
    assert stats() == before  # nothing above ran
    assert _state(lib, s0) == (M.SDPSK, 0)
    assert lib.srcdsp_mapper_destroy(s0) == capi.OK


@pytest.mark.parametrize("case", MAN["cases"], ids=[c["key"] for c in MAN["cases"]])
def test_step_host_of_a_host_handle_equals_the_reference(capi, case):
    """A handle that has never stepped on the device maps on the host, with
    the kernels' arithmetic (mapper_kernels.h): no device needed."""
    lib = capi.lib()
    h = _new(lib, case["kind"])
    for i, (bits, sym, state) in enumerate(M.golden_calls(case, ARR)):
        if i == case["copy_before"]:
            c = C.c_void_p()
            assert lib.srcdsp_mapper_clone(h, C.byref(c)) == 0 and lib.srcdsp_mapper_destroy(h) == 0
            h = c
        if i == case["reset_before"]:
            assert lib.srcdsp_mapper_reset(h) == 0
        b = np.ascontiguousarray(bits)
        out = np.full((len(sym) + 1, 2), 77, np.int16)  # one guard sample
        assert lib.srcdsp_mapper_step_host(h, b.ctypes.data, len(b), out.ctypes.data, len(sym)) == 0
        assert np.array_equal(out[:-1], sym) and (out[-1] == 77).all()
        assert _state(lib, h) == (case["kind"], state)
    assert lib.srcdsp_mapper_destroy(h) == 0


@pytest.fixture(scope="module")
def mapper_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mapper_host")
    exe = str(d / "mapper_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "mapper_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.parametrize("tile", [4096, 1, 7, 64])
def test_kernel_arithmetic_on_the_host_equals_the_reference(mapper_host, tile):
    """mapper_kernels.h compiled for the host under the address and
    undefined-behaviour sanitisers, the stream cut into tiles of `tile` bits
    (the scan's carry): every mapper golden byte for byte, and every state."""
    d, exe = mapper_host
    for case in MAN["cases"]:
        key = case["key"]
        (d / "case.bin").write_bytes(ARR[key + "_case"].tobytes())
        # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
        r = subprocess.run([exe, "case.bin", "out.bin", str(tile)], cwd=str(d), capture_output=True, text=True,
                           timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0 and not r.stderr.strip(), (key, r.stderr)
        assert (d / "out.bin").read_bytes() == ARR[key + "_out"].tobytes(), key
        assert [int(v) for v in r.stdout.split()] == case["states"], key


def _rows(tu, name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", tu), name, "400"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if name in ln]
    out = []
    for ln in rows:
        f = ln[ln.rindex(" VGPR "):].split()
        out.append({k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")})
    return out


def test_new_kernels_use_no_scratch():
    rows = _rows("mapper.hip", "mapper_")
    assert len(rows) == 5, rows  # tile parity, tile scan, the streaming kernel x (QPSK, SDPSK, SDPSK states)
    for row in rows:
        assert row["scratch"] == 0 and row["LDS"] <= 16 and row["VGPR"] <= 64, row
    rows = _rows("modulate.hip", "modulate_tile_dot2")
    assert len(rows) == 15, rows  # the shapes of upmix_tile_dot2
    for row in rows:
        assert row["scratch"] == 0, row
