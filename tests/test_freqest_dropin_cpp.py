"""The C++ drop-in include/srcdsp/dsptl_miscellaneous.h: estimateFreq<int16_t, L>
with the reference's signature, a DeviceSpan overload, and the two frequency
conversions.  CPU: the header compiles, alone and beside the other drop-ins,
and the conversions run.  GPU: tests/cpp/freqest_main.cpp, the program the
goldens were recorded with from the reference, built against the drop-in
reproduces every golden float bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import freqest_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include", "srcdsp")
LIBDIR = os.path.join(ROOT, "srcdsp_amd", "lib")
MAN, ARR = M.load_golden()


def _syntax(tmp_path, text, std="c++14"):
    src = tmp_path / "t.cpp"
    src.write_text(text)
    return subprocess.run(["g++", f"-std={std}", "-Wall", "-I", INC, "-fsyntax-only", str(src)],
                          capture_output=True, text=True)


def test_header_compiles(tmp_path):
    body = """
int main() {
    std::vector<std::complex<int16_t>> x(10);
    float f = estimateFreq<int16_t, 1>(x) + estimateFreq<int16_t, 32>(x);
    f += estimateFreq<int16_t, 2>(dsptl::DeviceSpan<const std::complex<int16_t>>{nullptr, 0});
    return (int)f + (int)dsptl::toFreqHz(0.1, 48000.0) + (int)dsptl::toFreqRadPerSample(100.0, 48000.0);
}
"""
    for std in ("gnu++11", "c++14"):
        r = _syntax(tmp_path, '#include "dsptl_miscellaneous.h"\n' + body, std)
        assert r.returncode == 0, r.stderr
    for a, b in (("demodulators.h", "dsptl_miscellaneous.h"), ("dsptl_miscellaneous.h", "correlators.h")):
        r = _syntax(tmp_path, f'#include "{a}"\n#include "{b}"\n' + body)
        assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", INC, "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "freqest_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_other_sample_types_do_not_compile(tmp_path):
    """The float instantiation is order-dependent and is left out: declared,
    not defined."""
    r = _syntax(tmp_path, '#include "dsptl_miscellaneous.h"\n'
                          "int main() { return (int)estimateFreq<float, 1>(std::vector<std::complex<float>>(4)); }\n")
    assert r.returncode != 0 and "EstimateFreq<float, 1>" in r.stderr


def test_conversions_run_without_the_library(tmp_path):
    src = tmp_path / "conv.cpp"
    src.write_text('#include "dsptl_miscellaneous.h"\n#include <cstdio>\n'
                   'int main() { std::printf("%.17g %.17g\\n", dsptl::toFreqHz(0.25, 48000.0), '
                   'dsptl::toFreqRadPerSample(1234.5, 48000.0)); return 0; }\n')
    exe = str(tmp_path / "conv")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-I", INC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hz, rad = (float(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert hz == 0.25 / 2.0 / np.pi * 48000.0 and rad == 2.0 * np.pi * 1234.5 / 48000.0


@pytest.fixture(scope="module")
def dropin_exe(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("freqest_dropin")
    exe = str(d / "freqest_main")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-I", INC, os.path.join(ROOT, "tests", "cpp", "freqest_main.cpp"),
                        "-o", exe, "-L", LIBDIR, "-lsrcdsp_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.gpu
def test_dropin_program_reproduces_the_goldens(dropin_exe):
    d, exe = dropin_exe
    args = []
    for c in MAN["cases"]:  # every case in one process: one HIP start-up
        x = np.ascontiguousarray(ARR[c["input"]][:c["n"]], np.int16)
        (d / (c["key"] + ".case")).write_bytes(struct.pack("<ii", c["L"], c["n"]) + x.tobytes())
        args += [c["key"] + ".case", c["key"] + ".out"]
    r = subprocess.run([exe] + args, cwd=str(d), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for c in MAN["cases"]:
        assert struct.unpack("<I", (d / (c["key"] + ".out")).read_bytes())[0] == c["bits"], c["key"]
