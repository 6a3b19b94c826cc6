"""The symbol mappers on the GPU (srcdsp_mapper_step, _step_host, _step_batched
and the Python classes): every golden recorded from the reference's
modulators.h, bit for bit with the state after every call; sizes around the
workgroup tile against the model; a stream in chunks; banks against the loop of
single calls; a guard band after every output row; and the C++ drop-in program
built against the library.

T = srcdsp_mapper_geometry's tile_bits (one workgroup: 256 lanes x 16 bits).
Outputs are compared as int16 [n, 2]."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapper_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include", "srcdsp")
LIBDIR = os.path.join(ROOT, "srcdsp_amd", "lib")
MAN, ARR = M.load_golden()
GUARD = 24  # samples after every output row that must stay untouched
BYTES = np.array(MAN["bit_bytes"], np.uint8)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def mapper(S, kind, state=0):
    m = (S.SymbolMapperQpsk if kind == M.QPSK else S.SymbolMapperSdpsk)()
    if state:
        m.setState(state)
    return m


def tile_bits(S):
    from srcdsp_amd import _capi as A
    t = C.c_int()
    A.call("srcdsp_mapper_geometry", C.byref(t))
    return t.value


def random_bits(n, seed):
    return np.random.default_rng(seed).choice(BYTES, n)


def step_guarded(S, m, bits_d, kind):
    """One device step into a buffer with a guard band; returns the symbols."""
    import torch
    n = bits_d.numel()
    ns = n // 2 if kind == M.QPSK else n
    out = torch.full((ns + GUARD, 2), 77, dtype=torch.int16, device="cuda")
    m.step(bits_d, out[:ns])
    y = out.cpu().numpy()
    assert (y[ns:] == 77).all()
    return y[:ns]


# ----------------------------------------------------------------- goldens
@pytest.mark.parametrize("path", ["device", "host", "mixed"])
@pytest.mark.parametrize("case", MAN["cases"], ids=[c["key"] for c in MAN["cases"]])
def test_goldens(S, case, path):
    """device: srcdsp_mapper_step; host: srcdsp_mapper_step_host on a handle
    that never touched the device; mixed: alternating, so that step_host also
    runs with the state on the device (staged through pinned memory)."""
    m = mapper(S, case["kind"])
    for i, (bits, sym, state) in enumerate(M.golden_calls(case, ARR)):
        if i == case["copy_before"]:
            m = copy.copy(m)
        if i == case["reset_before"]:
            m.reset()
        on_dev = path == "device" or (path == "mixed" and i % 2 == 0)
        if on_dev:
            y = step_guarded(S, m, dev(bits), case["kind"]) if len(bits) else m.step(dev(bits)).cpu().numpy()
        else:
            y = m.step(np.ascontiguousarray(bits))
        assert np.array_equal(y.reshape(-1, 2), sym), i
        assert m.state() == state, i


# ------------------------------------------------------------ around a tile
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_sizes_around_the_tile_vs_model(S, kind):
    T = tile_bits(S)
    assert T == 4096
    for k, n in enumerate((T - 2, T, T + 2, 3 * T + 6, T - 16)):
        for state in (0, 3):
            bits = random_bits(n, 100 * kind + k)
            ref = M.MapperModel(kind, state)
            want = ref.step(bits)
            m = mapper(S, kind, state)
            assert np.array_equal(step_guarded(S, m, dev(bits), kind), want), (n, state)
            assert m.state() == ref.state, (n, state)


@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_all_ones_and_all_zeros(S, kind):
    """Streams whose parity never / always flips, three tiles and a bit."""
    n = 3 * tile_bits(S) + 2
    for v in (0, 255):
        bits = np.full(n, v, np.uint8)
        ref = M.MapperModel(kind, 1)
        want = ref.step(bits)
        m = mapper(S, kind, 1)
        assert np.array_equal(step_guarded(S, m, dev(bits), kind), want)
        assert m.state() == ref.state


@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_stream_in_chunks_equals_one_call(S, kind):
    """(T + 2, 1, 2T - 3), each rounded up to even for QPSK; the later chunks
    start at byte offsets that are no multiple of 16."""
    T = tile_bits(S)
    chunks = [T + 2, 1, 2 * T - 3]
    if kind == M.QPSK:
        chunks = [n + n % 2 for n in chunks]
    bits = random_bits(sum(chunks), 7 + kind)
    bd = dev(bits)
    one = mapper(S, kind, 2)
    whole = step_guarded(S, one, bd, kind)
    assert np.array_equal(whole, M.MapperModel(kind, 2).step(bits))
    m = mapper(S, kind, 2)
    parts, pos = [], 0
    for n in chunks:
        parts.append(step_guarded(S, m, bd[pos:pos + n], kind))
        pos += n
    assert np.array_equal(np.concatenate(parts), whole)
    assert m.state() == one.state()


# -------------------------------------------------------------------- banks
def bank_call(S, ms, bits_d, bits_stride, out_d, out_stride, n_bits):
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles, _ptr, _stream
    A.call("srcdsp_mapper_step_batched", _handles(ms), len(ms), _ptr(bits_d), bits_stride, _ptr(out_d), out_stride,
           n_bits, _stream(bits_d))


@pytest.mark.parametrize("shared", [True, False], ids=["shared_bits", "padded_rows"])
@pytest.mark.parametrize("rows", [3, 65])
@pytest.mark.parametrize("kind", [M.SDPSK, M.QPSK])
def test_bank_equals_the_loop_of_single_calls(S, kind, rows, shared):
    """65 rows cross kMaxBatch = 64.  Start states differ per row."""
    import torch
    n, stride = 300, 320 if rows == 3 else 321  # padded; 321 is no multiple of 16 (no dwordx4 loads)
    ns = n // 2 if kind == M.QPSK else n
    bits = random_bits(stride * rows, 31 * rows + kind).reshape(rows, stride)
    bd = dev(bits[0, :n] if shared else bits)
    ms = [mapper(S, kind, c % 4) for c in range(rows)]
    singles = [copy.copy(m) for m in ms]
    for call in range(2):  # the second call starts from states the device holds
        out = torch.full((rows, ns + GUARD, 2), 77, dtype=torch.int16, device="cuda")
        bank_call(S, ms, bd, 0 if shared else stride, out, ns + GUARD, n)
        y = out.cpu().numpy()
        assert (y[:, ns:] == 77).all()
        for c in range(rows):
            row = bd if shared else bd[c, :n]
            assert np.array_equal(y[c, :ns], singles[c].step(row).cpu().numpy()), (call, c)
        assert [m.state() for m in ms] == [m.state() for m in singles], call
    # and the loop equals the model
    ref = M.MapperModel(kind, 1)
    ref.step(bits[0, :n] if shared else bits[1, :n])
    ref.step(bits[0, :n] if shared else bits[1, :n])
    assert ms[1].state() == ref.state


def test_python_bank_face(S):
    import torch
    bits = random_bits(3 * 64, 5).reshape(3, 64)
    ms = [mapper(S, M.SDPSK, c) for c in range(3)]
    out = torch.zeros((3, 64, 2), dtype=torch.int16, device="cuda")
    S.mapper_step_batched(ms, dev(bits), out)
    for c in range(3):
        assert np.array_equal(out[c].cpu().numpy(), M.MapperModel(M.SDPSK, c).step(bits[c]))
    S.mapper_step_batched(ms, dev(bits[0]), out)  # one shared row
    for c in range(3):
        r = M.MapperModel(M.SDPSK, c)
        r.step(bits[c])
        assert np.array_equal(out[c].cpu().numpy(), r.step(bits[0]))


# ------------------------------------------------------------------ drop-in
@pytest.fixture(scope="module")
def dropin_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mapper_dropin")
    exe = str(d / "mapper_main")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-I", INC, os.path.join(ROOT, "tests", "cpp", "mapper_main.cpp"),
                        "-o", exe, "-L", LIBDIR, "-lsrcdsp_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


def test_dropin_program_reproduces_the_goldens(S, dropin_exe):
    d, exe = dropin_exe
    keys = [c["key"] for c in MAN["cases"]]
    args = []
    for key in keys:  # every case in one process
        (d / (key + ".case")).write_bytes(ARR[key + "_case"].tobytes())
        args += [key + ".case", key + ".out"]
    r = subprocess.run([exe] + args, cwd=str(d), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for key in keys:
        assert (d / (key + ".out")).read_bytes() == ARR[key + "_out"].tobytes(), key
