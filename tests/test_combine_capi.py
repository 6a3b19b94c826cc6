"""CPU-side checks of the carrier combiner (srcdsp_combine_*): exported, in the
ctypes signature table and the header; the argument rules that refuse a call
before any HIP call; srcdsp_combine_step_host
against the numpy model; the kernel's arithmetic run on the host under
sanitisers; the C++ drop-in; the kernel's gfx950 resources -- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from combine_model import combine as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_combine_step", "srcdsp_combine_step_host")
DUMMY = C.c_void_p(4096)    # never dereferenced: every call it goes to is refused, or has nothing to do
DUMMY2 = C.c_void_p(1 << 20)
ROWS, NS, SHIFTS = (1, 2, 3, 64, 65, 1000), (0, 1, 7, 8, 9, 4099), (0, 1, 15)


@pytest.fixture(scope="module")
def capi():
    from srcdsp_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from srcdsp_amd.build import build
        build()
    return _capi


def carriers(rows, n, seed, stride=None):
    """int16 [rows, stride, 2]: random samples whose first columns hold what
    the clamp has to get right: every row at -32768 (the largest sum), every
    row at +32767, and sums that straddle each end of int16 at shift 0."""
    stride = n if stride is None else stride
    x = np.random.default_rng(seed).integers(-32768, 32768, (rows, stride, 2)).astype(np.int16)
    edge = [(-32768, 32767), (32767, -32768)]
    if rows >= 2:  # -32768 + -1 -> clamps; 32767 + 1 -> clamps; exactly at the ends -> does not
        edge += [(None, -32769, 32768), (None, -32768, 32767)]
    for i, e in enumerate(edge[:n]):
        if e[0] is None:
            x[:, i] = 0
            x[0, i] = (-32768, 32767)
            x[1, i] = (e[1] + 32768, e[2] - 32767)
        else:
            x[:, i] = e
    return x


def host(lib, x, n, shift, in_place=False):
    """srcdsp_combine_step_host over the rows of x [rows, stride, 2]."""
    rows, stride = x.shape[0], x.shape[1]
    if in_place:
        buf = x.copy()
        assert lib.srcdsp_combine_step_host(buf.ctypes.data, stride, rows, buf.ctypes.data, n, shift) == 0
        assert np.array_equal(buf[0, n:], x[0, n:]) and np.array_equal(buf[1:], x[1:])
        return buf[0, :n]
    out = np.full((n + 1, 2), 77, np.int16)  # one guard sample
    assert lib.srcdsp_combine_step_host(x.ctypes.data, stride, rows, out.ctypes.data, n, shift) == 0
    assert (out[-1] == 77).all()
    return out[:-1]


def test_library_exports_the_new_symbols(capi):
    lib = capi.lib()
    for s in NEW:
        assert s in capi.header_symbols(), s
        assert s in capi.SIGNATURES, s
        assert hasattr(lib, s), s
    assert len(capi.SIGNATURES["srcdsp_combine_step"][1]) == 7
    assert len(capi.SIGNATURES["srcdsp_combine_step_host"][1]) == 6
    with open(capi.HEADER) as f:
        text = f.read()
    sec = text[text.index("The carrier combiner"):text.index("FixedPatternCorrelator<int16_t, int32_t, N, S>")]
    assert sec.count("Extension") >= 2 and "dsp_complex.h:83-108" in sec and "row 0 itself" in sec


def test_python_face_is_exported():
    import srcdsp_amd
    assert "combine" in srcdsp_amd.__all__ and callable(srcdsp_amd.combine)


def test_model_definition():
    """The model against limitScale written out component by component."""
    x = carriers(3, 40, 1)
    for shift in SHIFTS:
        y = model(x, shift)
        for i in range(40):
            for k in range(2):
                a = (int(x[0, i, k]) + int(x[1, i, k]) + int(x[2, i, k])) >> shift
                assert y[i, k] == (32767 if a > 32767 else -32768 if a < -32768 else a)
    y = model(carriers(2, 8, 2), 0)
    assert y[:4].tolist() == [[-32768, 32767], [32767, -32768], [-32768, 32767], [-32768, 32767]]


def test_combine_refusals_come_before_any_device_call(capi):
    lib = capi.lib()
    for fn, tail in ((lib.srcdsp_combine_step, (None,)), (lib.srcdsp_combine_step_host, ())):
        assert fn(None, 8, 2, DUMMY2, 8, 0, *tail) == capi.ERR_ARG
        assert fn(DUMMY, 8, 2, None, 8, 0, *tail) == capi.ERR_ARG
        assert b"null buffer" in lib.srcdsp_last_error()
        assert fn(DUMMY, 8, 0, DUMMY2, 8, 0, *tail) == capi.ERR_ARG
        assert fn(DUMMY, 8, 65536, DUMMY2, 8, 0, *tail) == capi.ERR_ARG
        assert b"rows" in lib.srcdsp_last_error()
        assert fn(DUMMY, 8, 2, DUMMY2, 8, 16, *tail) == capi.ERR_ARG
        assert b"shift" in lib.srcdsp_last_error()
        # the rules hold when there is nothing to do, too
        assert fn(DUMMY, 8, 0, DUMMY2, 0, 0, *tail) == capi.ERR_ARG
        assert fn(DUMMY, 8, 2, DUMMY2, 0, 16, *tail) == capi.ERR_ARG
        # no samples: OK, nothing happens (null buffers are fine)
        assert fn(None, 0, 1, None, 0, 0, *tail) == capi.OK
        assert fn(DUMMY, 8, 65535, DUMMY2, 0, 15, *tail) == capi.OK


@pytest.mark.parametrize("rows", ROWS)
def test_step_host_equals_the_model(capi, rows):
    lib = capi.lib()
    for n in NS:
        x = carriers(rows, n, 10 * rows + n)
        for shift in SHIFTS:
            assert np.array_equal(host(lib, x, n, shift), model(x, shift)), (n, shift)
        assert np.array_equal(host(lib, x, n, 1, in_place=True), model(x, 1)), n


def test_step_host_saturates_at_both_ends(capi):
    """Both clamps occur, and the largest sum, rows * -32768, is exact."""
    lib = capi.lib()
    x = carriers(1000, 9, 3)
    y = host(lib, x, 9, 0)
    assert y[0].tolist() == [-32768, 32767] and y[1].tolist() == [32767, -32768]
    assert y[2].tolist() == [-32768, 32767] and y[3].tolist() == [-32768, 32767]  # one past each end, and at it
    y = host(lib, x, 9, 15)
    assert y[0].tolist() == [-1000, 999]  # (1000 * -32768) >> 15, (1000 * 32767) >> 15
    big = np.full((65535, 1, 2), -32768, np.int16)
    assert host(lib, big, 1, 15)[0].tolist() == [-32768, -32768]  # -65535: clamped, the sum did not wrap
    assert host(lib, big[:32768], 1, 15)[0].tolist() == [-32768, -32768]  # exactly -32768: not clamped
    assert host(lib, big[:32767], 1, 15)[0].tolist() == [-32767, -32767]


def test_step_host_strides(capi):
    """A stride wider than n, and in_stride == 0: the same row `rows` times."""
    lib = capi.lib()
    x = carriers(5, 23, 4, stride=23)
    assert np.array_equal(host(lib, x, 19, 2), model(x[:, :19], 2))
    row = carriers(1, 23, 5)
    out = np.zeros((23, 2), np.int16)
    assert lib.srcdsp_combine_step_host(row.ctypes.data, 0, 7, out.ctypes.data, 23, 1) == 0
    assert np.array_equal(out, model(np.repeat(row, 7, 0), 1))


def test_python_face_on_host_arrays():
    import srcdsp_amd as S
    x = carriers(3, 50, 6)
    assert np.array_equal(S.combine(x, shift=1), model(x, 1))
    assert np.array_equal(S.combine([x[0], x[1], x[2]]), model(x))
    assert np.array_equal(S.combine(x[0]), x[0])
    out = np.zeros((50, 2), np.int16)
    assert S.combine(x, out, 15) is out and np.array_equal(out, model(x, 15))


@pytest.fixture(scope="module")
def combine_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("combine_host")
    exe = str(d / "combine_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "combine_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.parametrize("rows", ROWS)
def test_kernel_arithmetic_on_the_host_equals_the_model(combine_host, rows):
    """combine_kernels.h compiled for the host under the address and
    undefined-behaviour sanitisers, on exactly sized buffers: the outputs byte
    for byte, also in place on row 0."""
    d, exe = combine_host
    for n in NS:
        stride = n + 3
        x = carriers(rows, n, 20 * rows + n, stride=stride)
        raw = x.reshape(-1, 2)[:(rows - 1) * stride + n]
        (d / "in.bin").write_bytes(raw.tobytes())
        for shift, in_place in ((0, 0), (1, 1), (15, 0)):
            # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
            r = subprocess.run([exe, "in.bin", "out.bin", str(rows), str(stride), str(n), str(shift), str(in_place)],
                               cwd=str(d), capture_output=True, text=True, timeout=120,
                               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
            assert r.returncode == 0 and not r.stderr.strip(), (n, shift, r.returncode, r.stderr)
            assert (d / "out.bin").read_bytes() == model(x[:, :n], shift).tobytes(), (n, shift)
    big = np.full((65535, 1, 2), -32768, np.int16)  # the largest sum: no signed overflow
    (d / "in.bin").write_bytes(big.tobytes())
    r = subprocess.run([exe, "in.bin", "out.bin", "65535", "1", "1", "15", "0"], cwd=str(d), capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    assert (d / "out.bin").read_bytes() == np.array([-32768, -32768], np.int16).tobytes()


def test_dropin_function_over_the_c_abi(capi, tmp_path):
    """dsptl::combineCarriers (include/srcdsp/modulators.h) through
    tests/cpp/combine_main.cpp: host vectors; rows of different sizes refused."""
    exe = str(tmp_path / "combine_main")
    libdir = os.path.dirname(capi.LIB_PATH)
    x = carriers(5, 37, 7)
    (tmp_path / "in.bin").write_bytes(x.tobytes())
    for std, extra in (("gnu++11", []), ("c++14", ["-DNDEBUG"])):
        r = subprocess.run(["g++", f"-std={std}", "-O1", "-Wall", *extra, "-I", os.path.join(ROOT, "include", "srcdsp"),
                            os.path.join(ROOT, "tests", "cpp", "combine_main.cpp"), "-L", libdir, "-lsrcdsp_hip",
                            f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for shift in (0, 2):
            r = subprocess.run([exe, "in.bin", "out.bin", "5", "37", str(shift)], cwd=str(tmp_path),
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.returncode, r.stderr)
            assert (tmp_path / "out.bin").read_bytes() == model(x, shift).tobytes()


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
    """combine_rows<4> and <1>: 8 int32 sums and four rows' (one row's) 16-byte
    loads per lane, no scratch, no LDS, registers for 8 waves per SIMD (DESIGN
    5.8b)."""
    rows = _rows("combine.hip", "combine_rows")
    assert len(rows) == 2, rows
    for row in rows:
        assert row["scratch"] == 0 and row["LDS"] == 0 and row["VGPR"] <= 64, rows
