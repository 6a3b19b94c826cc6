"""The C++ drop-in include/srcdsp/demodulators.h: dsptl::DemodulatorOqpsk<int16_t>
with the reference's public interface.  CPU: the header compiles, alone and
beside correlators.h.  GPU: tests/cpp/demod_main.cpp, the program the goldens
were recorded with from the reference, built against the drop-in reproduces
every golden output byte for byte."""
import os
import subprocess

import pytest

import demod_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include", "srcdsp")
LIBDIR = os.path.join(ROOT, "srcdsp_amd", "lib")
MAN, ARR = M.load_golden()


def _syntax(tmp_path, text, std="c++14"):
    src = tmp_path / "t.cpp"
    src.write_text(text)
    return subprocess.run(["g++", f"-std={std}", "-Wall", "-I", INC, "-fsyntax-only", str(src)],
                          capture_output=True, text=True)


def test_demodulators_header_compiles(tmp_path):
    body = """
int main() {
    dsptl::DemodulatorOqpsk<int16_t> d, e(d);
    e = d;
    d.setSyncPattern(std::vector<int8_t>{1, 0, 1});
    d.setReference(std::vector<std::complex<int16_t>>(3));
    d.setInitialFrequency(0.1f);
    d.setInitialPhase(0.2f);
    d.reset();
    d.setInputShift(2);
    int32_t error = 0;
    std::vector<int8_t> soft = d.step(std::vector<std::complex<int16_t>>(10), error);
    return (int)soft.size() + (int)d.getMeasuredFrequency();
}
"""
    for std in ("gnu++11", "c++14"):
        r = _syntax(tmp_path, '#include "demodulators.h"\n' + body, std)
        assert r.returncode == 0, r.stderr
    # the device-side reference from a correlator, with the headers in either order
    join = """
int main() {
    dsptl::FixedPatternCorrelator<int16_t, int32_t, 32, 1> corr;
    dsptl::DemodulatorOqpsk<int16_t> d;
    d.setReference(corr);
    int32_t error = 0;
    return (int)d.step(dsptl::DeviceSpan<const std::complex<int16_t>>{nullptr, 0}, dsptl::DeviceSpan<int8_t>{nullptr, 0},
                       error);
}
"""
    for a, b in (("correlators.h", "demodulators.h"), ("demodulators.h", "correlators.h")):
        r = _syntax(tmp_path, f'#include "{a}"\n#include "{b}"\n' + join)
        assert r.returncode == 0, r.stderr
    # tests/cpp/demod_main.cpp itself
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", INC, "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "demod_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def dropin_exe(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("demod_dropin")
    exe = str(d / "demod_main")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-I", INC, os.path.join(ROOT, "tests", "cpp", "demod_main.cpp"),
                        "-o", exe, "-L", LIBDIR, "-lsrcdsp_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


@pytest.mark.gpu
def test_dropin_program_reproduces_the_goldens(dropin_exe):
    d, exe = dropin_exe
    keys = [c["key"] for c in MAN["cases"]]
    args = []
    for key in keys:  # every case in one process: one HIP start-up
        (d / (key + ".case")).write_bytes(ARR[key + "_case"].tobytes())
        args += [key + ".case", key + ".out"]
    r = subprocess.run([exe] + args, cwd=str(d), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for key in keys:
        assert (d / (key + ".out")).read_bytes() == ARR[key + "_out"].tobytes(), key
