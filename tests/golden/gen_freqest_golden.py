#!/usr/bin/env python3
"""Goldens of the reference frequency estimator, estimateFreq<int16_t, L>
(dsptl_miscellaneous.h:43-58).

Compiles tests/cpp/freqest_main.cpp against the UNMODIFIED reference headers
where they lie (-I REF_DIR, in a temporary directory: nothing of the reference
is copied) with -fsanitize=address,undefined -fno-sanitize-recover=undefined,
runs it on every case below and stores the inputs in
tests/golden/freqest_golden.npz and, per case, the bit pattern of the returned
float in the manifest freqest_golden.json.  A case on which the sanitised
reference does not run clean stops the generator, so every committed input is
one on which the reference is defined (none holds -32768, where termI can
overflow int).

A case is a prefix of one of a few stored inputs: x = ARR[input][:n].

Run where the reference tree is:
    python tests/golden/gen_freqest_golden.py
"""
from __future__ import annotations

import json
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF_DIR", "/root/reference")
SRC = os.path.join(ROOT, "tests", "cpp", "freqest_main.cpp")

LS = (1, 2, 3, 4, 8, 32)
NMAX = 4097


def lengths(L):
    return sorted({0, 1, L, L + 1, 33, 257, 1000, NMAX})


def case_bin(L: int, x) -> bytes:
    x = np.ascontiguousarray(x, np.int16).reshape(-1, 2)
    return struct.pack("<ii", L, len(x)) + x.tobytes()


def inputs():
    rng = np.random.default_rng(20261)
    arr = {"noise": rng.integers(-32767, 32768, size=(NMAX, 2)).astype(np.int16),
           "full": (32767 * (2 * rng.integers(0, 2, size=(NMAX, 2)) - 1)).astype(np.int16)}
    om = {}
    j = np.arange(NMAX)
    for L in LS:
        om[L] = float(rng.uniform(-3.0 / L, 3.0 / L))
        th = float(rng.uniform(-3, 3))
        arr[f"tone_L{L}"] = np.stack([np.round(20000 * np.cos(th + om[L] * j)),
                                      np.round(20000 * np.sin(th + om[L] * j))], 1).astype(np.int16)
    return arr, om


def main():
    arr, om = inputs()
    meta = []
    flags = ["-std=gnu++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "freqest_ref")
        subprocess.run(["g++", *flags, "-I", REF, SRC, "-o", exe], check=True)
        for L in LS:
            for kind in ("noise", "full", "tone"):
                name = f"tone_L{L}" if kind == "tone" else kind
                for n in lengths(L):
                    key = f"{kind}_L{L}_n{n}"
                    with open(os.path.join(d, "case.bin"), "wb") as f:
                        f.write(case_bin(L, arr[name][:n]))
                    r = subprocess.run([exe, "case.bin", "out.bin"], cwd=d, capture_output=True, text=True,
                                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
                    if r.returncode != 0 or r.stderr.strip():
                        raise SystemExit(f"case {key}: the sanitised reference did not run clean ({r.returncode})\n"
                                         f"{r.stderr}")
                    with open(os.path.join(d, "out.bin"), "rb") as f:
                        (b,) = struct.unpack("<I", f.read())
                    c = {"key": key, "kind": kind, "L": L, "n": n, "input": name, "bits": b}
                    if kind == "tone":
                        c["omega"] = om[L]
                    meta.append(c)
                    print(c)
    np.savez_compressed(os.path.join(HERE, "freqest_golden.npz"), **arr)
    with open(os.path.join(HERE, "freqest_golden.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_freqest_golden.py",
                   "source": "reference dsptl_miscellaneous.h estimateFreq<int16_t, L> (g++ -O1 "
                             "-fsanitize=address,undefined, every case clean)",
                   "cases": meta}, f, indent=1)


if __name__ == "__main__":
    main()
