"""A/B of the carrier combiner's rows in flight: combine_rows<U>
forced to U = 1, 2, 4 and 8 for every shape, alternating in one process.

  python scripts/combine_ab.py --build    (needs hipcc and the product build's objects, no GPU)
      scripts/tune/ab/libsrcdsp_hip_combine_u<U>.so: the product's objects with
      combine.hip recompiled under -DSRCDSP_COMBINE_FORCE_ROWS_IN_FLIGHT=<U>
  python scripts/combine_ab.py [--out profiles/tuning/combine_rows_in_flight.json]    (needs a GPU)
      srcdsp_combine_step of each variant: 100 warm-up and 200 timed calls, HIP
      events on the launch stream, the variants alternating within every step
      and each timed twice; every variant's output is compared with U = 4's
      before timing.  Shapes: `long`, 2, 4 and 8 rows of 2^28, 2^27 and 2^26
      samples at a power-of-two stride and at one that is none; `grid`, rows in
      {2, 8, 16, 32, 64} x 2^16 ... 2^24 samples."""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
US = (1, 2, 4, 8)
PAD = 5 * 1024 + 4  # samples: a stride that is no power of two, rows still 16-byte aligned
LONG = [(2, 28, 0), (2, 28, PAD), (4, 27, 0), (4, 27, PAD), (8, 26, 0), (8, 26, PAD)]
GRID = [(r, lg, 0) for r in (2, 8, 16, 32, 64) for lg in (16, 18, 20, 22, 24)]


def lib_path(u):
    return os.path.join(ROOT, "scripts", "tune", "ab", f"libsrcdsp_hip_combine_u{u}.so")


def build():
    from srcdsp_amd import build as B
    B.build()
    src = os.path.join(B.CSRC, "combine.hip")
    rest = [os.path.join(B.OBJ, os.path.basename(s) + ".o") for s in sorted(glob.glob(os.path.join(B.CSRC, "*.hip")))
            if os.path.basename(s) != "combine.hip"]
    os.makedirs(os.path.dirname(lib_path(1)), exist_ok=True)
    for u in US:
        obj = os.path.join(B.OBJ + f"_combine_u{u}", "combine.hip.o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        for cmd in ([B._hipcc(), *B.CXXFLAGS, f"-DSRCDSP_COMBINE_FORCE_ROWS_IN_FLIGHT={u}", "-c", src, "-o", obj],
                    [B._hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", lib_path(u), *rest, obj, "-ldl",
                     f"-Wl,-rpath,{B.ROCM_LIB}"]):
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-4000:])
        print(lib_path(u))


def measure(a):
    import numpy as np
    import torch
    import srcdsp_amd as S
    from srcdsp_amd import _capi as A
    if not torch.cuda.is_available():
        raise SystemExit("combine_ab.py needs a GPU")
    libs = {}
    for u in US:
        lib = C.CDLL(lib_path(u))
        lib.srcdsp_combine_step.restype, lib.srcdsp_combine_step.argtypes = A.SIGNATURES["srcdsp_combine_step"]
        libs[f"u{u}"] = lib
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps, "unit": "ms per call",
           "protocol": "HIP events on the launch stream; u1, u2, u4, u8, then the four again, within every step",
           "long": {}, "grid": {}}
    for part, shapes in (("long", LONG), ("grid", GRID)):
        for rows, lg, pad in shapes:
            n = 1 << lg
            x = torch.empty((rows, n + pad, 2), dtype=torch.int16, device="cuda")
            S.fill_synthetic(x, "ci16", lo=-32767, hi=32767)
            ys = {k: torch.empty((n, 2), dtype=torch.int16, device="cuda") for k in libs}

            def mk(k):
                lib, y = libs[k], ys[k]

                def f():
                    if lib.srcdsp_combine_step(C.c_void_p(x.data_ptr()), n + pad, rows, C.c_void_p(y.data_ptr()), n, 2,
                                               sp) != 0:
                        raise SystemExit("srcdsp_combine_step failed")
                return f

            fns = {k + rep: mk(k) for rep in ("", "_again") for k in libs}
            for f in fns.values():
                f()
            torch.cuda.synchronize()
            if not all(torch.equal(ys["u4"], y) for y in ys.values()):
                raise SystemExit("the variants disagree")
            for _ in range(a.warmup):
                for f in fns.values():
                    f()
            ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(a.steps)] for k in fns}
            for i in range(a.steps):
                for k, f in fns.items():
                    e0, e1 = ev[k][i]
                    e0.record(st)
                    f()
                    e1.record(st)
            torch.cuda.synchronize()
            ms = {k: round(float(np.mean([e0.elapsed_time(e1) for e0, e1 in ev[k]])), 5) for k in fns}
            key = f"{rows}x2^{lg}" + (f"+{pad}" if pad else "")
            res[part][key] = ms
            print(key, ms, flush=True)
            del x, ys
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuning", "combine_rows_in_flight.json"))
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    build() if a.build else measure(a)
