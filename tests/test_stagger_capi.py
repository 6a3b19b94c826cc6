"""CPU-side checks of the Q-rail stagger and the offset modulator entry points
(srcdsp_stagger_*, srcdsp_modulate_offset_*): exported, in the ctypes signature
table and the header; the argument rules that refuse a call before any HIP call
with every handle's state unchanged; the handle's host-side behaviour (a
handle is a host object until it steps on the device) against the numpy model;
the kernels' arithmetic run on the host under sanitisers; the C++ drop-in; the
goldens against the oracle composition; the kernels' gfx950 resources -- no GPU
here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mapper_model as M
import stagger_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_stagger_create", "srcdsp_stagger_destroy", "srcdsp_stagger_clone", "srcdsp_stagger_reset",
       "srcdsp_stagger_get_state", "srcdsp_stagger_geometry", "srcdsp_stagger_step", "srcdsp_stagger_step_host",
       "srcdsp_stagger_step_batched", "srcdsp_modulate_offset_step", "srcdsp_modulate_offset_step_batched",
       "srcdsp_modulate_offset_stats")
DUMMY = C.c_void_p(4096)    # never dereferenced: every call it goes to is refused, or has nothing to do
DUMMY2 = C.c_void_p(1 << 20)
DS = (1, 2, 4, 7, 64)


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def _new(lib, D):
    h = C.c_void_p()
    assert lib.srcdsp_stagger_create(C.byref(h), D) == 0
    return h


def _state(lib, h):
    d = C.c_uint(0)
    carry = np.full(65, 77, np.int16)  # one guard value past the largest D
    assert lib.srcdsp_stagger_get_state(h, C.byref(d), carry.ctypes.data_as(C.POINTER(C.c_int16))) == 0
    assert (carry[d.value:] == 77).all()
    return d.value, carry[:d.value].tolist()


def _step_host(lib, h, x):
    x = np.ascontiguousarray(x, np.int16).reshape(-1, 2)
    out = np.full((len(x) + 1, 2), 77, np.int16)  # one guard sample
    assert lib.srcdsp_stagger_step_host(h, x.ctypes.data, len(x), out.ctypes.data) == 0
    assert (out[-1] == 77).all()
    return out[:-1]


def _samples(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, 2)).astype(np.int16)


def _prime(lib, h, D, seed):
    """A carry that is not zeros, and the model that holds the same."""
    m = G.StaggerModel(D)
    x = _samples(D + 3, seed)
    assert np.array_equal(_step_host(lib, h, x), m.step(x))
    return m


def test_library_exports_the_new_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_stagger_step"][1]) == 5
    assert len(capi.SIGNATURES["srcdsp_stagger_step_batched"][1]) == 8
    assert len(capi.SIGNATURES["srcdsp_modulate_offset_step"][1]) == 11
    assert len(capi.SIGNATURES["srcdsp_modulate_offset_step_batched"][1]) == 12
    with open(capi.HEADER) as f:
        text = f.read()
    # every new entry is marked as an extension and cites the reference calls it sits between
    sec = text[text.index("The OQPSK Q-rail stagger"):text.index("FixedPatternCorrelator<int16_t, int32_t, N, S>")]
    assert sec.count("Extension") >= 9 and "upsampling_filters.h:149-233" in sec and "mixers.h:169-188" in sec


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("QStagger", "stagger_step_batched", "stagger_geometry", "OffsetModulatorChain",
                 "modulate_offset_step", "modulate_offset_step_batched", "modulate_offset_stats"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name


def test_geometry(capi):
    t, d = C.c_int(), C.c_uint()
    assert capi.lib().srcdsp_stagger_geometry(C.byref(t), C.byref(d)) == 0
    assert (t.value, d.value) == (1024, 64)  # 256 lanes x one 16-byte load of 4 samples


def test_null_handles_and_bad_delays_are_refused(capi):
    lib = capi.lib()
    h = C.c_void_p()
    assert lib.srcdsp_stagger_create(None, 4) == capi.ERR_ARG
    for D in (0, 65, 1 << 20):
        assert lib.srcdsp_stagger_create(C.byref(h), D) == capi.ERR_ARG and not h.value
    assert lib.srcdsp_stagger_clone(None, C.byref(h)) == capi.ERR_ARG
    assert lib.srcdsp_stagger_reset(None) == capi.ERR_ARG
    assert lib.srcdsp_stagger_get_state(None, None, None) == capi.ERR_ARG
    assert lib.srcdsp_stagger_step(None, DUMMY, 4, DUMMY2, None) == capi.ERR_ARG
    assert lib.srcdsp_stagger_step_host(None, DUMMY, 4, DUMMY2) == capi.ERR_ARG
    assert lib.srcdsp_modulate_offset_step(None, None, None, None, DUMMY, 4, DUMMY2, 16, 0, 0, None) == capi.ERR_ARG
    g = _new(lib, 4)
    assert lib.srcdsp_modulate_offset_step(None, None, g, None, DUMMY, 4, DUMMY2, 16, 0, 0, None) == capi.ERR_ARG
    assert lib.srcdsp_stagger_destroy(g) == capi.OK
    assert lib.srcdsp_stagger_destroy(None) == capi.OK
    assert lib.srcdsp_last_error()


@pytest.mark.parametrize("D", DS)
def test_handle_lives_on_the_host_until_it_steps(capi, D):
    """create, step_host, reset, get_state and clone make no HIP call (this
    test runs where there is no device)."""
    lib = capi.lib()
    h = _new(lib, D)
    assert _state(lib, h) == (D, [0] * D)
    m = _prime(lib, h, D, 1)
    assert _state(lib, h) == (D, m.carry.tolist()) and any(m.carry)
    c = C.c_void_p()
    assert lib.srcdsp_stagger_clone(h, C.byref(c)) == capi.OK and _state(lib, c) == (D, m.carry.tolist())
    assert lib.srcdsp_stagger_reset(h) == capi.OK and _state(lib, h) == (D, [0] * D)
    assert _state(lib, c) == (D, m.carry.tolist())  # a value copy
    x = _samples(9, 2)
    assert np.array_equal(_step_host(lib, c, x), m.step(x))
    assert lib.srcdsp_stagger_destroy(h) == capi.OK and lib.srcdsp_stagger_destroy(c) == capi.OK


def test_step_refusals_change_nothing(capi):
    lib = capi.lib()
    h = _new(lib, 4)
    m = _prime(lib, h, 4, 3)
    buf = np.zeros((64, 2), np.int16)
    p = buf.ctypes.data
    for fn, tail in ((lib.srcdsp_stagger_step, (None,)), (lib.srcdsp_stagger_step_host, ())):
        assert fn(h, None, 8, DUMMY2, *tail) == capi.ERR_ARG
        assert fn(h, DUMMY, 8, None, *tail) == capi.ERR_ARG
        # overlap: in place, out one sample ahead, out one sample behind, the last byte shared
        assert fn(h, C.c_void_p(p), 8, C.c_void_p(p), *tail) == capi.ERR_ARG
        assert fn(h, C.c_void_p(p), 8, C.c_void_p(p + 4), *tail) == capi.ERR_ARG
        assert fn(h, C.c_void_p(p + 4), 8, C.c_void_p(p), *tail) == capi.ERR_ARG
        assert fn(h, C.c_void_p(p), 8, C.c_void_p(p + 31), *tail) == capi.ERR_ARG
        assert b"overlap" in lib.srcdsp_last_error()
        # no samples: OK, and nothing changes (null buffers are fine)
        assert fn(h, None, 0, None, *tail) == capi.OK
    assert _state(lib, h) == (4, m.carry.tolist())
    # adjacent buffers do not overlap
    x = _samples(8, 4)
    buf[:8] = x
    assert lib.srcdsp_stagger_step_host(h, C.c_void_p(p), 8, C.c_void_p(p + 32)) == capi.OK
    assert np.array_equal(buf[8:16], m.step(x)) and _state(lib, h) == (4, m.carry.tolist())
    assert lib.srcdsp_stagger_destroy(h) == capi.OK


def test_batched_argument_rules(capi):
    lib = capi.lib()
    step = lib.srcdsp_stagger_step_batched
    a, b, d = _new(lib, 4), _new(lib, 4), _new(lib, 5)
    models = [_prime(lib, h, D, 5 + i) for i, (h, D) in enumerate(((a, 4), (b, 4), (d, 5)))]
    two = (C.c_void_p * 2)(a.value, b.value)
    for ch in (0, -3):
        assert step(two, ch, DUMMY, 0, DUMMY2, 8, 8, None) == capi.ERR_ARG
    assert step(None, 2, DUMMY, 0, DUMMY2, 8, 8, None) == capi.ERR_ARG
    assert step((C.c_void_p * 2)(a.value, None), 2, DUMMY, 0, DUMMY2, 8, 8, None) == capi.ERR_ARG
    assert step((C.c_void_p * 2)(a.value, a.value), 2, DUMMY, 0, DUMMY2, 8, 8, None) == capi.ERR_ARG  # listed twice
    assert b"once" in lib.srcdsp_last_error()
    assert step((C.c_void_p * 2)(a.value, d.value), 2, DUMMY, 0, DUMMY2, 8, 8, None) == capi.ERR_ARG  # D differs
    assert b"share D" in lib.srcdsp_last_error()
    assert step(two, 2, DUMMY, 7, DUMMY2, 8, 8, None) == capi.ERR_ARG      # 0 < in_stride < n
    assert step(two, 2, DUMMY, 8, DUMMY2, 7, 8, None) == capi.ERR_SIZE     # out_stride < n
    assert step(two, 2, None, 8, DUMMY2, 8, 8, None) == capi.ERR_ARG
    assert step(two, 2, DUMMY, 8, None, 8, 8, None) == capi.ERR_ARG
    # the second output row reaches into the input rows
    assert step(two, 2, C.c_void_p(8192), 8, C.c_void_p(8192 - 40), 8, 8, None) == capi.ERR_ARG
    assert b"overlap" in lib.srcdsp_last_error()
    assert step(two, 2, None, 0, None, 0, 0, None) == capi.OK              # no samples
    for h, m in zip((a, b, d), models):
        assert _state(lib, h) == (m.D, m.carry.tolist())
        assert lib.srcdsp_stagger_destroy(h) == capi.OK


def test_modulate_offset_batched_refuses_missing_and_repeated_handles(capi):
    """The rules that need no interpolator or mixer (those are device objects
    from their creation; tests/test_gpu_modulate_offset.py has the rest)."""
    lib = capi.lib()
    step = lib.srcdsp_modulate_offset_step_batched

    def stats():
        v = [C.c_ulong(7) for _ in range(4)]
        assert lib.srcdsp_modulate_offset_stats(*[C.byref(x) for x in v]) == capi.OK
        return [x.value for x in v]

    before = stats()
    mp = C.c_void_p()
    assert lib.srcdsp_mapper_create(C.byref(mp), M.QPSK) == 0 and lib.srcdsp_mapper_set_state(mp, 2) == 0
    g = _new(lib, 4)
    m = _prime(lib, g, 4, 8)
    one_m, one_g = (C.c_void_p * 1)(mp.value), (C.c_void_p * 1)(g.value)
    none, fake = (C.c_void_p * 1)(None), (C.c_void_p * 1)(4096)
    args = (1, DUMMY, 0, DUMMY2, 64, 8, 0, None)
    assert step(None, fake, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, None, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, None, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, one_g, None, *args) == capi.ERR_ARG
    assert step(one_m, fake, one_g, fake, 0, *args[1:]) == capi.ERR_ARG
    assert step(none, fake, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, none, one_g, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, none, fake, *args) == capi.ERR_ARG
    assert step(one_m, fake, one_g, none, *args) == capi.ERR_ARG
    mp2 = C.c_void_p()
    assert lib.srcdsp_mapper_create(C.byref(mp2), M.QPSK) == 0
    two_m, fake2 = (C.c_void_p * 2)(mp.value, mp2.value), (C.c_void_p * 2)(4096, 8192)
    twice = (C.c_void_p * 2)(g.value, g.value)
    assert step(two_m, fake2, twice, fake2, 2, *args[1:]) == capi.ERR_ARG  # a stagger listed twice
    assert b"once" in lib.srcdsp_last_error()
    assert stats() == before  # nothing above ran
    assert _state(lib, g) == (4, m.carry.tolist())
    k, s = C.c_int(), C.c_int()
    assert lib.srcdsp_mapper_get_state(mp, C.byref(k), C.byref(s)) == 0 and s.value == 2
    assert lib.srcdsp_stagger_destroy(g) == capi.OK
    assert lib.srcdsp_mapper_destroy(mp) == capi.OK and lib.srcdsp_mapper_destroy(mp2) == capi.OK


@pytest.mark.parametrize("D", DS)
def test_step_host_equals_the_model(capi, D):
    """n in {0, 1, D-1, D, D+1, 1000}, in one call and split in two, from a
    carry that is not zeros."""
    lib = capi.lib()
    for k, n in enumerate((0, 1, D - 1, D, D + 1, 1000)):
        x = _samples(n, 10 * D + k)
        for cut in sorted({0, 1, n // 3, max(n - 1, 0), n}):
            if cut > n:
                continue
            h = _new(lib, D)
            m = _prime(lib, h, D, 100 + k)
            want = m.step(x)
            got = np.concatenate([_step_host(lib, h, x[:cut]), _step_host(lib, h, x[cut:])])
            assert np.array_equal(got, want), (n, cut)
            assert _state(lib, h) == (D, m.carry.tolist()), (n, cut)
            assert lib.srcdsp_stagger_destroy(h) == capi.OK


def test_model_definition():
    """The model against the definition written out sample by sample."""
    for D in (1, 3, 8):
        m = G.StaggerModel(D, np.arange(1, D + 1))
        x = _samples(D + 5, D)
        y = m.copy().step(x)
        for i in range(len(x)):
            assert y[i, 0] == x[i, 0] and y[i, 1] == (x[i - D, 1] if i >= D else i + 1)
        short = m.copy()
        short.step(x[:D - 1])  # n < D: the carry's tail moves up, the new values follow
        assert short.carry.tolist() == [D] + x[:D - 1, 1].tolist()


@pytest.fixture(scope="module")
def stagger_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("stagger_host")
    exe = str(d / "stagger_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "stagger_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.parametrize("D", DS)
def test_kernel_arithmetic_on_the_host_equals_the_model(stagger_host, D):
    """stagger_kernels.h compiled for the host under the address and
    undefined-behaviour sanitisers: outputs byte for byte, the carry after
    every call."""
    d, exe = stagger_host
    calls = [D + 1, 0, 1, D - 1, D, 1000, 3]
    x = _samples(sum(calls), 40 + D)
    (d / "in.bin").write_bytes(x.tobytes())
    # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
    r = subprocess.run([exe, str(D), "in.bin", "out.bin", *map(str, calls)], cwd=str(d), capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    m, pos, ys, carries = G.StaggerModel(D), 0, [], []
    for n in calls:
        ys.append(m.step(x[pos:pos + n]))
        carries.append(m.carry.tolist())
        pos += n
    assert (d / "out.bin").read_bytes() == np.concatenate(ys).tobytes()
    assert [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()] == carries


def test_dropin_class_over_the_c_abi(capi, tmp_path):
    """dsptl::QStagger (include/srcdsp/modulators.h) through tests/cpp/stagger_main.cpp:
    host vectors, a value copy and a reset in mid-stream."""
    exe = str(tmp_path / "stagger_main")
    libdir = os.path.dirname(capi.LIB_PATH)
    for std in ("gnu++11", "c++14"):
        r = subprocess.run(["g++", f"-std={std}", "-O1", "-Wall", "-I", os.path.join(ROOT, "include", "srcdsp"),
                            os.path.join(ROOT, "tests", "cpp", "stagger_main.cpp"), "-L", libdir, "-lsrcdsp_hip",
                            f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    D, calls = 4, [7, 3, 0, 50, 2, 9]
    x = _samples(sum(calls), 50)
    (tmp_path / "in.bin").write_bytes(x.tobytes())
    r = subprocess.run([exe, str(D), "in.bin", "out.bin", "2", "4", *map(str, calls)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m, pos, ys = G.StaggerModel(D), 0, []
    for c, n in enumerate(calls):
        if c == 4:
            m.reset()
        ys.append(m.step(x[pos:pos + n]))
        pos += n
    assert (tmp_path / "out.bin").read_bytes() == np.concatenate(ys).tobytes()


def test_goldens_equal_the_oracle_composition(O):
    """The goldens were recorded from the reference build's interpolator and
    mixer; the oracle's, with the mapper and stagger models, give the same."""
    man, arr = G.load_golden()
    assert len(man["chains"]) == 8
    assert {(c["L"], c["kind"], c["flush"][1]) for c in man["chains"]} == \
        {(L, k, f) for L in (4, 8) for k in (M.SDPSK, M.QPSK) for f in (False, True)}
    for ch in man["chains"]:
        k = ch["key"]
        bits, pos, calls = arr[k + "_bits"], 0, []
        for n, fl in zip(ch["calls"], ch["flush"]):
            calls.append((bits[pos:pos + n], fl))
            pos += n
        mapper, stag = M.MapperModel(ch["kind"]), G.StaggerModel(ch["D"])
        y = G.offset_chain(O["strict"], mapper, arr[k + "_taps"], ch["L"], stag, ch["freq"], calls, N=ch["N"])
        assert np.array_equal(y, arr[k + "_out"]), k
        assert np.array_equal(stag.carry, arr[k + "_carry"]) and mapper.state == ch["mapper_state"], k


def _rows(tu, name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", tu), name, "400"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for ln in (ln for ln in r.stdout.splitlines() if name in ln):
        f = ln[ln.rindex(" VGPR "):].split()
        out.append({k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch", "LDS")})
    return out


def test_new_kernels_use_no_scratch():
    rows = _rows("stagger.hip", "stagger_stream")
    assert len(rows) == 1 and rows[0]["scratch"] == 0 and rows[0]["VGPR"] <= 32, rows
    rows = _rows("modulate_offset.hip", "modoffset_tile_dot2")
    assert len(rows) == 15, rows  # the shapes of modulate_tile_dot2
    for row in rows:
        assert row["scratch"] == 0, row
