"""Time the SDPSK demodulator (srcdsp_sdpsk_step, srcdsp_sdpsk_step_batched).
The protocol of scripts/carrier_sum_time.py: one process, device-resident data,
HIP events on the launch stream, 100 warm-up steps, mean of 200 timed steps; the
alternatives alternate within every step and each is timed twice per round, so
its own run-to-run spread is on record.  Needs a GPU (no fallback).

Long rows: one row of 2^26 and one of 2^28 samples at D = 1, soft bits only
(4 B read and 1 B written per sample) and both outputs (2 B written).  Beside
them in the same process: srcdsp_freqest_run at L = 1, which reads the same
4 B per sample; what an application does today, the same product, shift and
clamp in torch; and, where they were built, the kernel at 4 and at 16 words per
lane (the product has 8).  The same row from 1 sample past a 16-byte boundary
(`off1`): the product's realigning 16-byte loads against the build whose rows
off a 16-byte boundary go sample by sample.

Banks: 64 and 1024 rows of 4096 samples out of one buffer (in_stride == 0, all
the hits of one stream), at offsets that are multiples of 4 samples and at odd
ones, against the loop of single calls; and, where it was built, the bank whose
rows off a 16-byte boundary go sample by sample instead of through the
realigning 16-byte loads.

  python scripts/sdpsk_time.py --build     (needs hipcc, no GPU)
      scripts/tune/ab/libsrcdsp_hip_sdpsk_{w4,w16,scalar}.so: the product's
      objects with sdpsk.hip recompiled under -DSRCDSP_SDPSK_LANE_WORDS=4 / 16,
      or -DSRCDSP_SDPSK_UNALIGNED_SCALAR
  python scripts/sdpsk_time.py [--out profiles/sdpsk_time.json] [--warmup 100] [--steps 200]
  python scripts/sdpsk_time.py --table     (the README's table from the JSON)"""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = {"w4": "SRCDSP_SDPSK_LANE_WORDS=4", "w16": "SRCDSP_SDPSK_LANE_WORDS=16",
            "scalar": "SRCDSP_SDPSK_UNALIGNED_SCALAR"}
SHIFT = 17
NAMES = ("srcdsp_sdpsk_create", "srcdsp_sdpsk_step", "srcdsp_sdpsk_step_batched")


def lib_path(v):
    return os.path.join(ROOT, "scripts", "tune", "ab", f"libsrcdsp_hip_sdpsk_{v}.so")


def build():
    from srcdsp_amd import build as B
    B.build()
    src = os.path.join(B.CSRC, "sdpsk.hip")
    rest = [os.path.join(B.OBJ, os.path.basename(s) + ".o") for s in sorted(glob.glob(os.path.join(B.CSRC, "*.hip")))
            if os.path.basename(s) != "sdpsk.hip"]
    os.makedirs(os.path.dirname(lib_path("w4")), exist_ok=True)
    for v, define in VARIANTS.items():
        obj = os.path.join(B.OBJ + f"_sdpsk_{v}", "sdpsk.hip.o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        for cmd in ([B._hipcc(), *B.CXXFLAGS, f"-D{define}", "-c", src, "-o", obj],
                    [B._hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", lib_path(v), *rest, obj, "-ldl",
                     f"-Wl,-rpath,{B.ROCM_LIB}"]):
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-4000:])
        print(lib_path(v))


def timed(fns, warmup, steps):
    """fns: {name: callable}.  Mean ms per call of each, the callables
    alternating within every step."""
    import numpy as np
    import torch
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k in fns}
    for i in range(steps):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record(st)
            fn()
            b.record(st)
    torch.cuda.synchronize()
    return {k: float(np.mean([a.elapsed_time(b) for a, b in ev[k]])) for k in fns}


def both_runs(fns):
    out = dict(fns)
    out.update({k + "_again": v for k, v in fns.items()})
    return out


def summary(ms, n_samples, bytes_of):
    """Per alternative: the faster of its two timings, their difference, and
    TB/s over its algorithmic bytes (None: not a streaming figure)."""
    out = {}
    for k in [k for k in ms if not k.endswith("_again")]:
        best = min(ms[k], ms[k + "_again"])
        out[k] = {"ms": round(best, 5), "spread_ms": round(abs(ms[k] - ms[k + "_again"]), 5)}
        if bytes_of.get(k):
            out[k]["bytes_per_sample"] = bytes_of[k]
            out[k]["TB_per_s"] = round(bytes_of[k] * n_samples / (1e-3 * best) / 1e12, 4)
    return out


class Lib:
    """The demodulator's entry points of the product library or of a variant."""

    def __init__(self, path=None):
        from srcdsp_amd import _capi as A
        self.lib = A.lib() if path is None else C.CDLL(path)
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = A.SIGNATURES[name]

    def handle(self, D=1, shift=SHIFT):
        h = C.c_void_p()
        if self.lib.srcdsp_sdpsk_create(C.byref(h), D, shift) != 0:
            raise SystemExit("srcdsp_sdpsk_create failed")
        return h

    def step(self, h, x, n, soft, bits, sp):
        if self.lib.srcdsp_sdpsk_step(h, x, n, soft, bits, sp) != 0:
            raise SystemExit("srcdsp_sdpsk_step failed")

    def bank(self, hs, rows, x, offs, n, soft, stride, sp):
        if self.lib.srcdsp_sdpsk_step_batched(hs, rows, x, 0, offs, n, soft, stride, None, 0, sp) != 0:
            raise SystemExit("srcdsp_sdpsk_step_batched failed")


def measure_long(libs, lg, a):
    import torch
    import srcdsp_amd as S
    n = 1 << lg
    x = torch.empty((n, 2), dtype=torch.int16, device="cuda")
    S.fill_synthetic(x, "ci16", lo=-32767, hi=32767)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp = C.c_void_p(x.data_ptr())
    soft = {k: torch.empty(n, dtype=torch.int8, device="cuda") for k in libs}
    bits = {k: torch.empty(n, dtype=torch.uint8, device="cuda") for k in libs}
    hs = {k: lib.handle() for k, lib in libs.items()}
    fe = S.FreqEstimator(1)

    def torch_form(want_bits):
        p, q = x[1:].to(torch.int32), x[:-1].to(torch.int32)
        tq = p[:, 1] * q[:, 0] - p[:, 0] * q[:, 1]
        s = (tq >> SHIFT).clamp(-128, 127).to(torch.int8)
        return (s, (tq > 0).to(torch.uint8)) if want_bits else (s, None)

    for k, lib in libs.items():
        lib.step(hs[k], xp, n, C.c_void_p(soft[k].data_ptr()), C.c_void_p(bits[k].data_ptr()), sp)
    m = 1 << 20  # a spot check of 2^20 outputs against torch, then the variants against the product
    p, q = x[1:m + 1].to(torch.int32), x[:m].to(torch.int32)
    tq = p[:, 1] * q[:, 0] - p[:, 0] * q[:, 1]
    if not (torch.equal(soft["w8"][1:m + 1], (tq >> SHIFT).clamp(-128, 127).to(torch.int8))
            and torch.equal(bits["w8"][1:m + 1], (tq > 0).to(torch.uint8))):
        raise SystemExit("the demodulator and torch disagree")
    if not all(torch.equal(soft[v][1:], soft["w8"][1:]) and torch.equal(bits[v][1:], bits["w8"][1:]) for v in libs):
        raise SystemExit("the variants disagree")

    def mk(v, want_bits):
        lib, h, s, b = libs[v], hs[v], C.c_void_p(soft[v].data_ptr()), C.c_void_p(bits[v].data_ptr())
        return lambda: lib.step(h, xp, n, s, b if want_bits else None, sp)

    def mk_off1(v):  # n - 4 samples from 1 sample past the boundary
        lib, h, s = libs[v], libs[v].handle(), C.c_void_p(soft[v].data_ptr())
        return lambda: lib.step(h, C.c_void_p(x.data_ptr() + 4), n - 4, s, None, sp)

    fns = {}
    for v in libs:
        if v != "scalar":
            fns[f"sdpsk_{v}_soft"] = mk(v, False)
            fns[f"sdpsk_{v}_both"] = mk(v, True)
        if v in ("w8", "scalar"):
            fns[f"sdpsk_{v}_soft_off1"] = mk_off1(v)
    fns["freqest"] = lambda: fe.run(x)
    fns["torch_soft"] = lambda: torch_form(False)
    fns["torch_both"] = lambda: torch_form(True)
    if "scalar" in libs:
        fns["sdpsk_w8_soft_off1"]()
        fns["sdpsk_scalar_soft_off1"]()
        torch.cuda.synchronize()
        if not torch.equal(soft["w8"][:n - 4], soft["scalar"][:n - 4]):
            raise SystemExit("the two forms of a row off a 16-byte boundary disagree")
    bytes_of = {k: (6 if k.endswith("_both") else 5) for k in fns if k.startswith("sdpsk_")}
    bytes_of["freqest"] = 4
    ms = timed(both_runs(fns), a.warmup, a.steps)
    r = {"samples": n, "D": 1, "shift": SHIFT, "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
         "alternatives": summary(ms, n, bytes_of)}
    alt = r["alternatives"]
    r["ratios"] = {f"{mode}_over_{other}": round(alt[f"sdpsk_w8_{mode}"]["ms"] / alt[other]["ms"], 4)
                   for mode in ("soft", "both") for other in ("freqest", f"torch_{mode}")}
    if "sdpsk_scalar_soft_off1" in alt:
        r["ratios"]["soft_off1_over_scalar_soft_off1"] = round(alt["sdpsk_w8_soft_off1"]["ms"]
                                                               / alt["sdpsk_scalar_soft_off1"]["ms"], 4)
    r["ratios"]["soft_off1_over_soft"] = round(alt["sdpsk_w8_soft_off1"]["ms"] / alt["sdpsk_w8_soft"]["ms"], 4)
    r["TB_per_s_over_freqest"] = {mode: round(alt[f"sdpsk_w8_{mode}"]["TB_per_s"] / alt["freqest"]["TB_per_s"], 4)
                                  for mode in ("soft", "both")}
    print(json.dumps(r), flush=True)
    return r


def measure_bank(libs, rows, odd, a):
    import torch
    import srcdsp_amd as S
    n, pitch = 4096, 4100  # a hit every 4100 samples
    offs_l = [c * pitch + (2 * (c % 2) + 1 if odd else 0) for c in range(rows)]
    x = torch.empty((rows * pitch + n + 8, 2), dtype=torch.int16, device="cuda")
    S.fill_synthetic(x, "ci16", lo=-32767, hi=32767)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    offs = (C.c_size_t * rows)(*offs_l)
    use = {k: v for k, v in libs.items() if k in ("w8", "scalar")}
    soft = {k: torch.zeros((rows, n), dtype=torch.int8, device="cuda") for k in list(use) + ["loop"]}
    hv = {k: [lib.handle() for _ in range(rows)] for k, lib in use.items()}
    hv["loop"] = [libs["w8"].handle() for _ in range(rows)]
    arr = {k: (C.c_void_p * rows)(*[h.value for h in v]) for k, v in hv.items()}

    def bank(k):
        lib, hs, s = use[k], arr[k], C.c_void_p(soft[k].data_ptr())
        return lambda: lib.bank(hs, rows, C.c_void_p(x.data_ptr()), offs, n, s, n, sp)

    def loop():
        lib, base, s0 = libs["w8"], x.data_ptr(), soft["loop"].data_ptr()
        for c in range(rows):
            lib.step(hv["loop"][c], C.c_void_p(base + 4 * offs_l[c]), n, C.c_void_p(s0 + c * n), None, sp)

    fns = {f"bank_{k}": bank(k) for k in use}
    fns["loop_of_single_calls"] = loop
    for _ in range(2):  # the second call starts from the carry every later one starts from
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    if not all(torch.equal(s, soft["w8"]) for s in soft.values()):
        raise SystemExit("the bank, its variant and the loop disagree")
    ms = timed(both_runs(fns), a.warmup, a.steps)
    bytes_of = {k: 5 for k in fns if k.startswith("bank_")}
    r = {"rows": rows, "samples_per_row": n, "offsets": "odd" if odd else "multiples of 4 samples", "in_stride": 0,
         "ms_per_call": {k: round(v, 5) for k, v in ms.items()}, "alternatives": summary(ms, rows * n, bytes_of)}
    alt = r["alternatives"]
    r["ratios"] = {"bank_over_loop": round(alt["bank_w8"]["ms"] / alt["loop_of_single_calls"]["ms"], 4)}
    if "bank_scalar" in alt:
        r["ratios"]["bank_over_bank_scalar"] = round(alt["bank_w8"]["ms"] / alt["bank_scalar"]["ms"], 4)
    print(json.dumps(r), flush=True)
    return r


def measure(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sdpsk_time.py needs a GPU")
    libs = {"w8": Lib()}
    for v in VARIANTS:
        if os.path.exists(lib_path(v)):
            libs[v] = Lib(lib_path(v))
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "protocol": "HIP events on the launch stream; the alternatives alternate per step, each timed twice; means",
           "alternatives": {"sdpsk_w8": "the product, 8 words per lane", "sdpsk_w4 / sdpsk_w16": "4 / 16 words per lane",
                            "bank_scalar": "rows off a 16-byte boundary sample by sample",
                            "torch": "the same product, shift and clamp in torch",
                            "freqest": "srcdsp_freqest_run, L = 1, 4 B read per sample"},
           "long": {}, "bank": {}}
    for lg in (26, 28):
        res["long"][f"2^{lg}"] = measure_long(libs, lg, a)
        torch.cuda.empty_cache()
    for rows in (64, 1024):
        for odd in (False, True):
            res["bank"][f"{rows}x4096_{'odd' if odd else 'aligned'}"] = measure_bank(libs, rows, odd, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def table(a):
    with open(a.out) as f:
        res = json.load(f)
    print("| shape | outputs | ms | TB/s | x freqest's time | x torch's time |")
    print("|---|---|---|---|---|---|")
    for key, r in res["long"].items():
        for mode in ("soft", "both"):
            alt = r["alternatives"][f"sdpsk_w8_{mode}"]
            print(f"| 1 x {key} | {mode} | {alt['ms']:.4f} | {alt['TB_per_s']:.2f} | "
                  f"{r['ratios'][f'{mode}_over_freqest']:.2f} | {r['ratios'][f'{mode}_over_torch_{mode}']:.3f} |")
    for key, r in res["bank"].items():
        alt = r["alternatives"]["bank_w8"]
        print(f"| {key.replace('_', ', ')} offsets | soft | {alt['ms']:.4f} | {alt['TB_per_s']:.2f} | - | "
              f"loop of single calls: {r['ratios']['bank_over_loop']:.4f} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdpsk_time.json"))
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    build() if a.build else table(a) if a.table else measure(a)
