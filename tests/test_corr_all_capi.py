"""CPU-side checks of srcdsp_corr_step_all: exported, in the ctypes signature
table and the header; the argument rules that refuse a call before any HIP
call; the walk of csrc/corr_all_walk.h run on the host under sanitisers
(tests/cpp/corr_all_host.cpp) against the oracle loop on every case the GPU
test runs; the candidate kernel's gfx950 resources -- no GPU here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import corr_all_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srcdsp_corr_step_all", "srcdsp_corr_step_all_host", "srcdsp_corr_step_all_batched", "srcdsp_corr_all_stats")
CASES = M.cases()


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
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert [len(capi.SIGNATURES[s][1]) for s in NEW] == [9, 8, 11, 2]


def test_python_face_is_exported():
    import srcdsp_amd
    for name in ("corr_step_all_batched", "corr_all_stats"):
        assert name in srcdsp_amd.__all__ and callable(getattr(srcdsp_amd, name)), name
    assert callable(srcdsp_amd.FixedPatternCorrelator.stepAll)


def test_null_arrays_counts_and_max_hits_are_argument_errors(capi):
    lib = capi.lib()
    one = (C.c_void_p * 1)(None)
    k, idx, used = (C.c_int * 1)(), (C.c_int * 4)(), (C.c_size_t * 1)()
    for hs, a, b, c in ((None, k, idx, used), (one, None, idx, used), (one, k, None, used), (one, k, idx, None),
                        (one, k, idx, used)):  # the last: a null handle in the list
        assert lib.srcdsp_corr_step_all_batched(hs, 1, None, 0, 0, 4, a, b, None, c, None) == capi.ERR_ARG
        assert lib.srcdsp_last_error()
    for ch in (0, -3):
        assert lib.srcdsp_corr_step_all_batched(one, ch, None, 0, 0, 4, k, idx, None, used, None) == capi.ERR_ARG
    for mh in (0, -1):
        assert lib.srcdsp_corr_step_all_batched(one, 1, None, 0, 0, mh, k, idx, None, used, None) == capi.ERR_ARG
        assert b"max_hits" in lib.srcdsp_last_error()
    assert lib.srcdsp_corr_step_all(None, None, 0, 4, k, idx, None, used, None) == capi.ERR_ARG
    assert lib.srcdsp_corr_step_all_host(None, None, 0, 4, k, idx, None, used) == capi.ERR_ARG


def test_stats_are_zero_in_a_fresh_process(capi):
    code = ("from srcdsp_amd import _capi as A; import ctypes as C; b, l = C.c_ulong(7), C.c_ulong(7); "
            "assert A.lib().srcdsp_corr_all_stats(C.byref(b), C.byref(l)) == 0; print(b.value, l.value)")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "0"]


@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("corr_all_host")
    exe = str(d / "corr_all_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "corr_all_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.parametrize("batch", [3, 1024])
@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_on_the_host_equals_the_oracle_loop(O, walk_host, name, batch):
    """corr_all_walk.h compiled for the host under the address and
    undefined-behaviour sanitisers, in patch batches of 3 values (every batch
    boundary taken) and of the kernel's 1024: indices, bit rows, consumed and
    the registers after every call, the history at the end."""
    d, exe = walk_host
    N, p, x, chunks, mh = CASES[name]
    ref = O["fma"].corr(N, 1)
    ref.set_pattern(p)
    st = []

    def call(xs, m):
        out = M.step_all(ref, xs, m)
        st.append(ref.status())
        return out

    want = M.run_calls(call, x, chunks, mh)
    assert sum(len(w[1]) for w in want) >= 1, name
    (d / "p.bin").write_bytes(np.ascontiguousarray(p, np.int32).tobytes())
    (d / "x.bin").write_bytes(np.ascontiguousarray(x, np.int16).tobytes())
    # a stand-alone host program; the leak check needs ptrace, which a sandbox may deny
    r = subprocess.run([exe, str(N), str(st[0]["coeff_scaling"]), str(mh), str(batch), "p.bin", "x.bin",
                        *map(str, chunks)], cwd=str(d), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    heads = [ln for ln in lines if ln[0] == "H"]
    idxs = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "I"]
    rows = [np.array(ln[1:], np.int64).reshape(N, 2) for ln in lines if ln[0] == "B"]
    assert len(heads) == len(want) == len(idxs)
    deleted, pos_rows = [], 0
    for h, ix, w, s in zip(heads, idxs, want, st):
        assert (int(h[1]), int(h[2])) == (len(w[1]), w[3]) and ix == w[1], (name, w[0], h, ix, w[1])
        assert [int(v) for v in h[3:6]] == s["corr"] and [int(v) for v in h[6:9]] == s["energy"], (name, w[0])
        for k in range(len(w[1])):
            assert np.array_equal(rows[pos_rows + k], w[2][k]), (name, w[0], k)
        pos_rows += len(w[1])
        deleted += [w[0] + i + 1 for i in w[1]]
    assert pos_rows == len(rows)
    # the history: the last N - 1 samples processed and not detected
    kept = np.delete(x[:sum(chunks)], deleted, axis=0)[-(N - 1):]
    tail = np.array([ln for ln in lines if ln[0] == "T"][0][1:], np.int64).reshape(-1, 2)
    assert np.array_equal(tail, kept), name


def build_dropin(capi, exe, stds=("gnu++11", "c++14")):
    libdir = os.path.dirname(capi.LIB_PATH)
    for std in stds:
        r = subprocess.run(["g++", f"-std={std}", "-O1", "-Wall", "-I", os.path.join(ROOT, "include", "srcdsp"),
                            os.path.join(ROOT, "tests", "cpp", "corr_all_main.cpp"), "-L", libdir, "-lsrcdsp_hip",
                            f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_dropin_member_compiles_against_the_library(capi, tmp_path):
    """dsptl::FixedPatternCorrelator::stepAll (include/srcdsp/correlators.h); it runs in test_gpu_corr_all.py."""
    build_dropin(capi, str(tmp_path / "corr_all_main"))


def _rows(src, name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"),
                        os.path.join("srcdsp_amd", "csrc", src), name],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if name + "(" in ln]
    assert len(rows) == 1, r.stdout + r.stderr[-2000:]
    f = rows[0]
    return {k: int(f[f.index(k) + 1]) for k in ("VGPR", "scratch")}


def test_candidate_kernel_uses_no_scratch_and_no_more_registers_than_the_scan():
    """corr_all_map is the scan's tile without its early exit: no scratch, and
    within corr_scan_s1's registers (the tile's occupancy is tuned)."""
    scan, cand = _rows("corr.hip", "corr_scan_s1"), _rows("corr_all.hip", "corr_all_map")
    assert cand["scratch"] == 0, cand
    assert cand["VGPR"] <= scan["VGPR"], (scan, cand)
