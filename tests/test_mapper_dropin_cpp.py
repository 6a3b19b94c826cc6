"""The C++ drop-in include/srcdsp/modulators.h: dsptl::SymbolMapperSdpsk<int16_t>
and dsptl::SymbolMapperQpsk<int16_t> with the reference's public interface.
The header compiles alone and beside upsampling_filters.h and mixers.h, in
either order, under gnu++11 and c++14; the other T are declared and not
defined.  (tests/test_gpu_mapper.py runs tests/cpp/mapper_main.cpp built
against it.)"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include", "srcdsp")

BODY = """
int main() {
    dsptl::SymbolMapperSdpsk<int16_t> s, s2(s);
    dsptl::SymbolMapperQpsk<int16_t> q, q2(q);
    s2 = s;
    q2 = q;
    std::vector<uint8_t> bits(8, 1);
    std::vector<std::complex<int16_t>> a(8), b(4);
    s.step(bits, a);
    q.step(bits, b);
    s.reset();
    q.reset();
    s.step(dsptl::DeviceSpan<const uint8_t>{nullptr, 0}, dsptl::DeviceSpan<std::complex<int16_t>>{nullptr, 0});
    q.step(dsptl::DeviceSpan<const uint8_t>{nullptr, 0}, dsptl::DeviceSpan<std::complex<int16_t>>{nullptr, 0}, nullptr);
    return (int)a.size() + (int)b.size() + (s.handle() != nullptr) + (q2.handle() != nullptr);
}
"""


def _syntax(tmp_path, text, std):
    src = tmp_path / "t.cpp"
    src.write_text(text)
    return subprocess.run(["g++", f"-std={std}", "-Wall", "-I", INC, "-fsyntax-only", str(src)],
                          capture_output=True, text=True)


@pytest.mark.parametrize("std", ["gnu++11", "c++14"])
def test_modulators_header_compiles_alone_and_beside_the_chain_headers(tmp_path, std):
    r = _syntax(tmp_path, '#include "modulators.h"\n' + BODY, std)
    assert r.returncode == 0, r.stderr
    for order in itertools.permutations(("modulators.h", "upsampling_filters.h", "mixers.h")):
        r = _syntax(tmp_path, "".join(f'#include "{h}"\n' for h in order) + BODY, std)
        assert r.returncode == 0, (order, r.stderr)
    r = subprocess.run(["g++", f"-std={std}", "-Wall", "-I", INC, "-fsyntax-only",
                        os.path.join(ROOT, "tests", "cpp", "mapper_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("T", ["float", "double", "int8_t", "int32_t"])
def test_other_component_types_are_declared_and_not_defined(tmp_path, T):
    for cls in ("SymbolMapperSdpsk", "SymbolMapperQpsk"):
        ok = _syntax(tmp_path, f'#include "modulators.h"\ndsptl::{cls}<{T}> *p = nullptr;\nint main() {{ return p != nullptr; }}\n',
                     "c++14")
        assert ok.returncode == 0, ok.stderr
        bad = _syntax(tmp_path, f'#include "modulators.h"\nint main() {{ dsptl::{cls}<{T}> m; return 0; }}\n', "c++14")
        assert bad.returncode != 0 and "incomplete type" in bad.stderr, bad.stderr
