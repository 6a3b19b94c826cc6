#!/usr/bin/env python3
"""Goldens of the reference symbol mappers (modulators.h) and of the transmit
chain mapper -> FilterUpsamplingFir -> Mixer built from the reference classes.

Compiles tests/cpp/mapper_main.cpp (with -DMAPPER_OPEN_STATE, which opens the
private `state` member after the standard headers are in) and the small chain
driver below against the UNMODIFIED reference headers where they lie
(-I REF_DIR, in a temporary directory: nothing of the reference is copied) with
plain g++ and -fsanitize=address,undefined, runs them on every case and stores
the case files and what the programs wrote in tests/golden/mapper_golden.npz,
with the manifest mapper_golden.json.  A case on which the sanitised reference
does not run clean stops the generator.

Run where the reference tree is:
    python tests/golden/gen_mapper_golden.py
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF_DIR", "/root/reference")
SRC = os.path.join(ROOT, "tests", "cpp", "mapper_main.cpp")
sys.path.insert(0, os.path.join(ROOT, "tests"))

BIT_BYTES = np.array([0, 1, 2, 128, 255], np.uint8)  # every non-zero byte is a one

# mapper -> interpolator -> mixer from the reference's own classes.
#   chain <case.bin> <out.bin>
# case.bin: int32 kind, int32 L, float freq, int32 ntaps, int32 taps[ntaps],
#           int32 n0, int32 n1 (bits of the two calls), uint8 bits
# out.bin: the two calls' samples, int16 (re, im); the second call flushes.
CHAIN_SRC = r"""
#include <cmath>
#include <cassert>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>
#include <array>
#include "modulators.h"
#include "upsampling_filters.h"
#include "mixers.h"
typedef std::complex<int16_t> ci16;
typedef std::complex<int32_t> ci32;
template <class T> static T get(std::ifstream &f) { T v{}; f.read((char *)&v, sizeof v); return v; }

template <class Mapper, unsigned L>
static int run(std::ifstream &f, int div, const char *out_path) {
    const float freq = get<float>(f);
    std::vector<int32_t> taps((size_t)get<int32_t>(f));
    for (auto &t : taps) t = get<int32_t>(f);
    const int32_t n[2] = {get<int32_t>(f), get<int32_t>(f)};
    std::vector<uint8_t> bits((size_t)n[0] + n[1]);
    f.read((char *)bits.data(), bits.size());
    if (!f) return 3;
    Mapper mapper;
    dsptl::FilterUpsamplingFir<ci16, ci16, ci32, int32_t, L> up(taps);
    dsptl::Mixer<ci16, ci16, int16_t, 4096> mixer;
    mixer.setFrequency(freq);
    std::ofstream out(out_path, std::ios::binary);
    size_t pos = 0;
    for (int c = 0; c < 2; ++c) {
        const bool flush = c == 1;
        const std::vector<uint8_t> b(bits.begin() + pos, bits.begin() + pos + n[c]);
        pos += n[c];
        std::vector<ci16> sym(b.size() / div);
        mapper.step(b, sym);
        std::vector<ci16> tmp(sym.size() * L + (flush ? L * (up.getLength() / L) : 0)), y(tmp.size());
        up.step(sym, tmp, flush);
        mixer.step(tmp, y);
        for (const auto &s : y) {
            const int16_t v[2] = {s.real(), s.imag()};
            out.write((const char *)v, 4);
        }
    }
    return out.good() ? 0 : 4;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const int32_t kind = get<int32_t>(f), L = get<int32_t>(f);
    if (kind == 0 && L == 4) return run<dsptl::SymbolMapperSdpsk<int16_t>, 4>(f, 1, argv[2]);
    if (kind == 0 && L == 2) return run<dsptl::SymbolMapperSdpsk<int16_t>, 2>(f, 1, argv[2]);
    if (kind == 1 && L == 4) return run<dsptl::SymbolMapperQpsk<int16_t>, 4>(f, 2, argv[2]);
    if (kind == 1 && L == 2) return run<dsptl::SymbolMapperQpsk<int16_t>, 2>(f, 2, argv[2]);
    return 2;
}
"""


def mapper_cases(rng):
    out = []
    for kind, name in ((0, "sdpsk"), (1, "qpsk")):
        even = (lambda n: n - n % 2) if kind == 1 else (lambda n: n)

        def add(key, calls, reset_before=-1, copy_before=-1):
            calls = [even(n) for n in calls]
            out.append({"key": f"{name}_{key}", "kind": kind, "calls": calls, "reset_before": reset_before,
                        "copy_before": copy_before, "bits": rng.choice(BIT_BYTES, sum(calls))})

        for n in (0, 1, 2, 3, 255, 256, 257):
            if kind == 1 and n % 2:
                continue
            add(f"n{n}", [n])
        add("chunks", [5 + kind, 130, 67], )          # three unequal calls, the state carried across
        add("reset", [41, 50, 8], reset_before=1)      # reset() between calls
        add("copy", [30, 45], copy_before=1)           # a value copy carries the state
        add("empty_mid", [21, 0, 12])                  # a step of no bits leaves the state
    return out


def chain_cases(rng):
    out = []
    for kind, name in ((0, "sdpsk"), (1, "qpsk")):
        for L, ntaps, freq, nsym in ((4, 16, 0.1137, (150, 173)), (2, 10, -0.3021, (97, 204))):
            taps = rng.integers(-2000, 2001, ntaps).astype(np.int32)
            per = 2 if kind == 1 else 1
            calls = [n * per for n in nsym]
            out.append({"key": f"chain_{name}_L{L}", "kind": kind, "L": L, "freq": freq, "taps": taps,
                        "calls": calls, "bits": rng.choice(BIT_BYTES, sum(calls))})
    return out


def run_clean(cmd, cwd, what):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0 or r.stderr.strip():
        raise SystemExit(f"{what}: the sanitised reference did not run clean ({r.returncode})\n{r.stderr}")


def main():
    import mapper_model as M
    rng = np.random.default_rng(20261)
    arrays, meta, chains = {}, [], []
    flags = ["-std=gnu++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    with tempfile.TemporaryDirectory() as d:
        exe, chain = os.path.join(d, "mapper_ref"), os.path.join(d, "chain_ref")
        subprocess.run(["g++", *flags, "-DMAPPER_OPEN_STATE", "-I", REF, SRC, "-o", exe], check=True)
        with open(os.path.join(d, "chain.cpp"), "w") as f:
            f.write(CHAIN_SRC)
        subprocess.run(["g++", *flags, "-I", REF, os.path.join(d, "chain.cpp"), os.path.join(REF, "dsp_complex.cpp"),
                        "-o", chain], check=True)
        for c in mapper_cases(rng):
            k = c["key"]
            blob = M.case_bin(c["kind"], c["reset_before"], c["copy_before"], c["calls"], c["bits"])
            with open(os.path.join(d, "case.bin"), "wb") as f:
                f.write(blob)
            run_clean([exe, "case.bin", "out.bin"], d, k)
            with open(os.path.join(d, "out.bin"), "rb") as f:
                ob = f.read()
            states = np.fromfile(os.path.join(d, "out.bin.state"), "<i4")
            sym = M.parse_out(ob, len(c["calls"]))
            arrays[k + "_case"] = np.frombuffer(blob, np.uint8)
            arrays[k + "_out"] = np.frombuffer(ob, np.uint8)
            arrays[k + "_bits"] = c["bits"]
            arrays[k + "_sym"] = np.concatenate(sym) if sym else np.zeros((0, 2), np.int16)
            meta.append({"key": k, "kind": c["kind"], "calls": c["calls"], "reset_before": c["reset_before"],
                         "copy_before": c["copy_before"], "states": [int(s) for s in states]})
            print(meta[-1])
        for c in chain_cases(rng):
            k = c["key"]
            blob = struct.pack("<iifi", c["kind"], c["L"], c["freq"], len(c["taps"])) + c["taps"].tobytes()
            blob += struct.pack("<ii", *c["calls"]) + c["bits"].tobytes()
            with open(os.path.join(d, "case.bin"), "wb") as f:
                f.write(blob)
            run_clean([chain, "case.bin", "out.bin"], d, k)
            arrays[k + "_bits"], arrays[k + "_taps"] = c["bits"], c["taps"]
            arrays[k + "_out"] = np.fromfile(os.path.join(d, "out.bin"), np.int16).reshape(-1, 2)
            chains.append({"key": k, "kind": c["kind"], "L": c["L"], "N": 4096, "freq": c["freq"],
                           "ntaps": len(c["taps"]), "calls": c["calls"], "flush": [False, True]})
            print(chains[-1], arrays[k + "_out"].shape)
    np.savez_compressed(os.path.join(HERE, "mapper_golden.npz"), **arrays)
    with open(os.path.join(HERE, "mapper_golden.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_mapper_golden.py",
                   "source": "reference modulators.h, upsampling_filters.h, mixers.h "
                             "(g++ -O1 -fsanitize=address,undefined, every case clean)",
                   "bit_bytes": [int(b) for b in BIT_BYTES], "cases": meta, "chains": chains}, f, indent=1)


if __name__ == "__main__":
    main()
