"""A/B of where the summing modulator tile keeps a lane's 2 * 8 L int32 sums
(DESIGN 5.8c): registers against the lane's own column of an int32 tile in
LDS, modsum_tile_dot2 forced to either for L = 2 and L = 4 (at L = 8 the LDS
tile would be 128 KiB beside a 70 KiB output tile: registers only),
alternating in one process.

  python scripts/modulate_sum_ab.py --build    (needs hipcc and the product build's objects, no GPU)
      scripts/tune/ab/libsrcdsp_hip_modsum_{regs,lds}.so: the product's objects
      with modulate_sum.hip recompiled under -DSRCDSP_MODSUM_FORCE_LDS_SUMS={0,1};
      prints the kernels' resources of both
  python scripts/modulate_sum_ab.py [--out profiles/tuning/modulate_sum_sums.json]    (needs a GPU)
      srcdsp_modulate_sum_step of each variant with the routing threshold at
      one tile: 100 warm-up and 200 timed calls, HIP events on the launch
      stream, the variants alternating within every step and each timed twice;
      the variants' wires are compared before timing.  Shapes: (a) and (d) of
      scripts/carrier_sum_time.py, and 8 carriers x 2^23 symbols at L = 2, 32
      taps; QPSK and SDPSK."""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
VARIANTS = {"regs": 0, "lds": 1}
SHAPES = {"a": dict(C=8, n=1 << 23, L=4, ntaps=128), "d": dict(C=2, n=1 << 25, L=4, ntaps=64),
          "l2": dict(C=8, n=1 << 23, L=2, ntaps=32)}


def lib_path(name):
    return os.path.join(ROOT, "scripts", "tune", "ab", f"libsrcdsp_hip_modsum_{name}.so")


def build():
    from srcdsp_amd import build as B
    B.build()
    src = os.path.join(B.CSRC, "modulate_sum.hip")
    rest = [os.path.join(B.OBJ, os.path.basename(s) + ".o") for s in sorted(glob.glob(os.path.join(B.CSRC, "*.hip")))
            if os.path.basename(s) != "modulate_sum.hip"]
    os.makedirs(os.path.dirname(lib_path("regs")), exist_ok=True)
    for name, v in VARIANTS.items():
        obj = os.path.join(B.OBJ + f"_modsum_{name}", "modulate_sum.hip.o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        define = f"-DSRCDSP_MODSUM_FORCE_LDS_SUMS={v}"
        for cmd in ([B._hipcc(), *B.CXXFLAGS, define, "-c", src, "-o", obj],
                    [B._hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", lib_path(name), *rest, obj, "-ldl",
                     f"-Wl,-rpath,{B.ROCM_LIB}"]):
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-4000:])
        print(lib_path(name))
        r = subprocess.run([B._hipcc(), *B.CXXFLAGS, define, "-c", src, "--offload-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull], capture_output=True, text=True)
        keep = ("Function Name", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy")
        for line in r.stderr.splitlines():
            if any(k in line for k in keep):
                print("  " + line.split("remark:")[-1].split("[-Rpass")[0].strip())


def measure(a):
    import torch
    import srcdsp_amd as S
    from carrier_sum_time import KINDS, SHIFT, timed
    from modulate_sum_time import chains
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles
    if not torch.cuda.is_available():
        raise SystemExit("modulate_sum_ab.py needs a GPU")
    libs = {}
    for name in VARIANTS:
        lib = C.CDLL(lib_path(name))
        for fn in ("srcdsp_modulate_sum_step", "srcdsp_modulate_sum_set_min_tiles", "srcdsp_modulate_sum_stats"):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = A.SIGNATURES[fn]
        if lib.srcdsp_modulate_sum_set_min_tiles(1) != 0:
            raise SystemExit("set_min_tiles failed")
        libs[name] = lib
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps, "unit": "ms per call",
           "protocol": "HIP events on the launch stream; regs, lds, then the two again, within every step", "shapes": {}}
    for key, sh in SHAPES.items():
        for kind, (_, bps) in KINDS.items():
            Cn, n, L = sh["C"], sh["n"], sh["L"]
            bits = torch.randint(0, 2, (Cn, bps * n), dtype=torch.uint8, device="cuda")
            wires = {k: torch.empty((L * n, 2), dtype=torch.int16, device="cuda") for k in libs}

            def mk(k, hs):
                lib, y, lists = libs[k], wires[k], [_handles(h) for h in hs]

                def f():
                    if lib.srcdsp_modulate_sum_step(*lists, Cn, C.c_void_p(bits.data_ptr()), bps * n,
                                                    C.c_void_p(y.data_ptr()), L * n, bps * n, 0, SHIFT, sp) != 0:
                        raise SystemExit("srcdsp_modulate_sum_step failed")
                f.keep = (hs, lists)
                return f

            first = {k: mk(k, chains(kind, Cn, L, sh["ntaps"])) for k in libs}  # the same step from the same start
            for k, f in first.items():
                v = [C.c_ulong(), C.c_ulong()]
                libs[k].srcdsp_modulate_sum_stats(C.byref(v[0]), C.byref(v[1]))
                f()
                w = [C.c_ulong(), C.c_ulong()]
                libs[k].srcdsp_modulate_sum_stats(C.byref(w[0]), C.byref(w[1]))
                if w[0].value != v[0].value + 1:
                    raise SystemExit(f"{k}: the fused kernel did not serve the call")
            torch.cuda.synchronize()
            if not torch.equal(wires["regs"], wires["lds"]):
                raise SystemExit("the variants disagree")
            fns = {k + rep: mk(k, chains(kind, Cn, L, sh["ntaps"])) for rep in ("", "_again") for k in libs}
            ms = {k: round(v, 5) for k, v in timed(fns, a.warmup, a.steps).items()}
            res["shapes"][f"{key}_{kind}"] = dict(sh, kind=kind, ms=ms)
            print(key, kind, ms, flush=True)
            del bits, wires, fns, first
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuning", "modulate_sum_sums.json"))
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    build() if a.build else measure(a)
