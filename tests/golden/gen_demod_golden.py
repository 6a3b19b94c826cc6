#!/usr/bin/env python3
"""Goldens of the reference OQPSK demodulator (demodulators.h/.cpp).

Compiles tests/cpp/demod_main.cpp against the UNMODIFIED reference headers
where they lie (-I REF_DIR, linked with its demodulators.cpp, in a temporary
directory: nothing of the reference is copied) with
-fsanitize=address,undefined -fno-sanitize-recover=undefined, runs it on every
case below and stores the case files and what the program wrote in
tests/golden/demod_golden.npz, with the manifest demod_golden.json.  A case
on which the sanitised reference does not run clean stops the generator, so
every committed input is one on which the reference is defined.

The two lookup tables (sine 8192, phase 128 x 128; 48 KiB of int16) are dumped
by a second small program of this generator that constructs the reference
object and writes its two member vectors.

Run where the reference tree is:
    python tests/golden/gen_demod_golden.py
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
SRC = os.path.join(ROOT, "tests", "cpp", "demod_main.cpp")
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = 64  # the kernel's tile length (samples per row and tile), demod_kernels.h kDemodTile

# the table dump: the class's private members opened after the standard headers
DUMP_SRC = r"""
#include <cmath>
#include <cassert>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <vector>
#define private public
#include "demodulators.h"
#undef private
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    dsptl::DemodulatorOqpsk<int16_t> d;
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    std::fwrite(d.sineLUT.data(), 2, d.sineLUT.size(), f);
    std::fwrite(d.phaseLUT.data(), 2, d.phaseLUT.size(), f);
    return std::fclose(f) == 0 ? 0 : 3;
}
"""


def case_bin(c) -> bytes:
    bits = np.ascontiguousarray(c["bits"], np.int8)
    ref = np.ascontiguousarray(c["ref"], np.int16).reshape(-1, 2)
    b = struct.pack("<i", len(bits)) + bits.tobytes() + struct.pack("<i", len(ref)) + ref.tobytes()
    b += struct.pack("<i", c["shift"]) + np.float32(c["freq"]).tobytes() + struct.pack("<i", c["reset_before"])
    b += struct.pack("<i", len(c["chunks"])) + np.asarray(c["chunks"], "<i4").tobytes()
    return b + np.ascontiguousarray(c["x"], np.int16).tobytes()


def cases():
    import demod_model as M
    rng = np.random.default_rng(20260)
    out = []

    def add(key, n_chunks, P=0, shift=0, word=13, amp=16000, x=None, ref=None, bits=None, reset_before=-1,
            ref_len=None):
        chunks = [n_chunks] if isinstance(n_chunks, int) else list(n_chunks)
        n = sum(chunks)
        if bits is None:
            bits = rng.integers(0, 2, P)
        if ref is None:
            ref = rng.integers(-amp, amp + 1, size=(P if ref_len is None else ref_len, 2))
        if x is None:
            x = rng.integers(-amp, amp + 1, size=(n, 2))
        out.append({"key": key, "P": int(P), "shift": shift, "word": word, "freq": M.word_freq(word), "chunks": chunks,
                    "reset_before": reset_before, "bits": np.asarray(bits, np.int8),
                    "ref": np.asarray(ref, np.int16), "x": np.asarray(x, np.int16)})

    for n in (1, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5):      # call lengths around 32 and the tile
        add(f"n{n}", n)
    for P in (2, 16, T + 3):                                    # preambles; T + 3 crosses a tile
        add(f"p{P}", 2 * T + 5, P=P)
        add(f"p{P}_first", [P + 1, 40], P=P)                    # the shortest first call, then a second
    for s in (0, 3, 8):                                         # arithmetic shifts of negative inputs
        add(f"shift{s}", 2 * T + 5, P=16, shift=s, amp=32767)
    for a in (100, 16000, 32767):                               # 32767: the int16 wrap in the rotation
        add(f"amp{a}", 2 * T + 5, word=-13, amp=a)
    for w in (0, 13, -13, 4096, -4096):
        add(f"word{w}", 2 * T + 5, P=2, word=w)
    add("chain", [70, 50, 13], P=16)                            # the third call measures frequency 0
    add("reset", [50, 60], P=16, shift=3, reset_before=1)       # reset(): shift back to 0, bits from the pattern
    add("longref", 2 * T + 5, P=16, ref_len=40)                 # a reference longer than the preamble
    # a burst the loop locks on: the signal model the demodulator itself
    # reconstructs, a carrier offset of 0.01 rad/sample (13 table steps), the
    # reference = the preamble's carrier
    P, nd, scale, om, th = 32, 2 * T + 40, 0.25, 0.01, 0.3
    bits = rng.integers(0, 2, P + nd)
    x = M.oqpsk_samples(bits, scale, om, th)
    add("locked", P + nd, P=P, shift=6, word=0, x=x, bits=bits[:P],
        ref=M.carrier_samples(P, scale * 23000, om, th))
    out[-1]["tx_bits"] = np.asarray(bits[P:], np.int8)
    return out


def parse_out(blob: bytes, n_chunks: int):
    soft, sizes, err, mf, pos = [], [], [], [], 0
    for _ in range(n_chunks):
        (ns,) = struct.unpack_from("<i", blob, pos)
        pos += 4
        soft.append(np.frombuffer(blob, np.int8, ns, pos))
        pos += ns
        (e,) = struct.unpack_from("<i", blob, pos)
        mf.append(np.frombuffer(blob, np.float32, 1, pos + 4)[0])
        pos += 8
        sizes.append(ns)
        err.append(e)
    assert pos == len(blob)
    return sizes, soft, err, mf


def main():
    arrays, meta = {}, []
    flags = ["-std=gnu++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    with tempfile.TemporaryDirectory() as d:
        exe, dump = os.path.join(d, "demod_ref"), os.path.join(d, "demod_tables")
        subprocess.run(["g++", *flags, "-I", REF, SRC, os.path.join(REF, "demodulators.cpp"), "-o", exe], check=True)
        with open(os.path.join(d, "dump.cpp"), "w") as f:
            f.write(DUMP_SRC)
        subprocess.run(["g++", *flags, "-I", REF, os.path.join(d, "dump.cpp"), os.path.join(REF, "demodulators.cpp"),
                        "-o", dump], check=True)
        subprocess.run([dump, os.path.join(d, "tables.bin")], check=True)
        tab = np.fromfile(os.path.join(d, "tables.bin"), np.int16)
        assert tab.size == 8192 + 128 * 128
        arrays["sine"], arrays["phase"] = tab[:8192].copy(), tab[8192:].copy()
        for c in cases():
            k = c["key"]
            blob = case_bin(c)
            with open(os.path.join(d, "case.bin"), "wb") as f:
                f.write(blob)
            r = subprocess.run([exe, "case.bin", "out.bin"], cwd=d, capture_output=True, text=True)
            if r.returncode != 0 or r.stderr.strip():
                raise SystemExit(f"case {k}: the sanitised reference did not run clean ({r.returncode})\n{r.stderr}")
            with open(os.path.join(d, "out.bin"), "rb") as f:
                ob = f.read()
            sizes, soft, err, mf = parse_out(ob, len(c["chunks"]))
            arrays[k + "_case"] = np.frombuffer(blob, np.uint8)
            arrays[k + "_out"] = np.frombuffer(ob, np.uint8)
            arrays[k + "_bits"], arrays[k + "_ref"], arrays[k + "_x"] = c["bits"], c["ref"], c["x"]
            arrays[k + "_freq"] = np.array([c["freq"]], np.float32)
            arrays[k + "_soft"] = np.concatenate(soft) if soft else np.zeros(0, np.int8)
            arrays[k + "_error"] = np.array(err, np.int32)
            arrays[k + "_mfreq"] = np.array(mf, np.float32)
            if "tx_bits" in c:
                arrays[k + "_tx_bits"] = c["tx_bits"]
            meta.append({"key": k, "P": c["P"], "shift": c["shift"], "word": c["word"], "chunks": c["chunks"],
                         "reset_before": c["reset_before"], "soft_sizes": sizes})
            print(meta[-1], "error", err)
    np.savez_compressed(os.path.join(HERE, "demod_golden.npz"), **arrays)
    with open(os.path.join(HERE, "demod_golden.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_demod_golden.py",
                   "source": "reference demodulators.h/.cpp (g++ -O1 -fsanitize=address,undefined, every case clean)",
                   "tile": T, "tables": {"sine": 8192, "phase": 128 * 128}, "cases": meta}, f, indent=1)


if __name__ == "__main__":
    main()
