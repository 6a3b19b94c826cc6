"""Time srcdsp_freqest_* and srcdsp_demod_acquire_batched.  One process,
device-resident data, 100 warm-up rounds, mean of 200 timed rounds.  An
estimator call returns its answer to the host, so every figure is wall-clock
time per call (the call's own synchronise included), taken between two device
synchronisations; alternatives alternate within a round and each is timed
twice, so the run-to-run spread is on record.  Needs a GPU (no fallback).

(s) One row of 2^26 and of 2^28 samples, L = 1 and L = 32: time, 4 n bytes /
    time, and that as a share of the 8 TB/s HBM specification.  Beside them, in
    the same process and protocol: FilterFir float -> complex<float>, 31 taps,
    on as many samples (12 bytes per sample), and what a user does today
    without the call: a D2H copy of the buffer and the host loop (the library's
    per-pair function, g++ -O2, one thread), --today-rounds rounds.
(b) A bank of 64 and of 1024 rows of 4096 samples: one batched call against
    the loop of single-row calls.
(j) The join for 64 and 1024 hits against the per-channel sequence
    set_reference_corr, get_bit_samples, a host estimate, set_initial_frequency,
    reset.  Both are host code.

Usage: python scripts/freqest_time.py [--out profiles/freqest_time.json] [--parts sbj]
       [--warmup 100] [--steps 200] [--today-rounds 3]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_SPEC = 8.0e12
HOST_SRC = r"""
#include "freqest_pair.h"
extern "C" void freqest_host_loop(const uint32_t *x, size_t n, size_t L, long long *out) {
    const srcdsp::FreqAcc a = srcdsp::freqest_row_host(x, n, L);
    out[0] = a.si; out[1] = a.sq; out[2] = a.hi; out[3] = a.lo;
}
"""


def host_loop(tmp):
    """The library's per-pair function over a host row: g++ -O2, one thread."""
    src, so = os.path.join(tmp, "loop.cpp"), os.path.join(tmp, "libloop.so")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "srcdsp_amd", "csrc"), src,
                    "-o", so], check=True)
    fn = C.CDLL(so).freqest_host_loop
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_longlong)]
    fn.restype = None

    def run(x: np.ndarray, L: int):
        out = (C.c_longlong * 4)()
        fn(x.ctypes.data, len(x), L, out)
        return out[0], out[1]
    return run


def timed(fns, warmup, steps, sync):
    """fns: {name: callable}; the callables alternate within a round."""
    t = {k: [] for k in fns}
    for i in range(warmup + steps):
        for k, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                t[k].append(time.perf_counter() - t0)
    return {k: 1e3 * float(np.mean(v)) for k, v in t.items()}


def stream(S, torch, a, loop):
    out = {}
    for lg in (26, 28):
        n = 1 << lg
        x = torch.empty((n, 2), dtype=torch.int16, device="cuda")
        S.fill_synthetic(x, "ci16", lo=-32767, hi=32767)
        e1, e32 = S.FreqEstimator(1), S.FreqEstimator(32)
        xf = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
        yf = torch.empty(n, dtype=torch.complex64, device="cuda")
        from srcdsp_amd.design import hamming_sinc
        fir = S.FilterFir(hamming_sinc(31, 0.2), "float", "complex<float>", "float", "float")
        ms = timed({"L1": lambda: e1.run(x), "L32": lambda: e32.run(x), "fir": lambda: fir.step(xf, yf),
                    "L1_again": lambda: e1.run(x), "L32_again": lambda: e32.run(x),
                    "fir_again": lambda: fir.step(xf, yf)}, a.warmup, a.steps, torch.cuda.synchronize)
        r = {"samples": n, "warmup": a.warmup, "steps": a.steps, "ms_per_call": {k: round(v, 5) for k, v in ms.items()}}
        for k in ("L1", "L32"):
            best = min(ms[k], ms[k + "_again"])
            r[k] = {"TB_per_s": round(4 * n / (1e-3 * best) / 1e12, 4), "share_of_8TBps": round(4 * n / (1e-3 * best) / HBM_SPEC, 4)}
        best = min(ms["fir"], ms["fir_again"])
        r["fir"] = {"bytes_per_sample": 12, "TB_per_s": round(12 * n / (1e-3 * best) / 1e12, 4),
                    "share_of_8TBps": round(12 * n / (1e-3 * best) / HBM_SPEC, 4)}
        # today: the buffer to the host (pinned), then the host loop
        del xf, yf
        h = torch.empty((n, 2), dtype=torch.int16).pin_memory()
        want = e1.run(x)[1]
        tc, tl = [], []
        for _ in range(a.today_rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.copy_(x)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            got = loop(h.numpy().view(np.uint32).reshape(-1), 1)
            tl.append(time.perf_counter() - t1)
            tc.append(t1 - t0)
            if got != want:
                raise SystemExit("the host loop and the kernel disagree")
        r["today_L1"] = {"rounds": a.today_rounds, "d2h_ms": round(1e3 * min(tc), 3), "host_loop_ms": round(1e3 * min(tl), 3),
                         "what": "hipMemcpy D2H into pinned memory, then freqest_pair over the row, g++ -O2, one thread; minima"}
        out[f"2^{lg}"] = r
        print(json.dumps({f"2^{lg}": r}), flush=True)
        del x, h
    return out


def bank(S, torch, a):
    out = {}
    for C_ in (64, 1024):
        n = 4096
        x = torch.empty((C_, n, 2), dtype=torch.int16, device="cuda")
        S.fill_synthetic(x, "ci16", lo=-32767, hi=32767)
        e = S.FreqEstimator(1)
        rows = [x[c] for c in range(C_)]

        def loop():
            return [e.run(r) for r in rows]
        f, sums, _ = e.run_batched(x)
        for c, (lf, ls, _) in enumerate(loop()):
            if ls != (int(sums[c, 0]), int(sums[c, 1])):
                raise SystemExit(f"bank {C_}: the batched call and the loop disagree on row {c}")
        steps = a.steps if C_ == 64 else max(a.steps // 10, 1)
        warm = a.warmup if C_ == 64 else max(a.warmup // 10, 1)
        ms = timed({"batched": lambda: e.run_batched(x), "loop": loop, "loop_again": loop}, warm, steps,
                   torch.cuda.synchronize)
        r = {"rows": C_, "samples_per_row": n, "L": 1, "warmup": warm, "steps": steps,
             "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
             "batched_over_loop": round(ms["batched"] / min(ms["loop"], ms["loop_again"]), 4)}
        out[str(C_)] = r
        print(json.dumps({f"bank {C_}": r}), flush=True)
    return out


def join(S, torch, a, loop):
    import copy
    out = {}
    N = 16
    pat = np.tile(np.array([[round(24324 / np.sqrt(N)), 0]], np.int32), (N, 1))
    for C_ in (64, 1024):
        rng = np.random.default_rng(C_)
        x = rng.integers(-125, 126, size=(C_, 256, 2)).astype(np.int32)
        j = np.arange(N)
        for c in range(C_):
            om, th = rng.uniform(0.0, 0.15), rng.uniform(-3, 3)
            x[c, 100:100 + N, 0] += np.round(2606 * np.cos(th + om * j)).astype(np.int32)
            x[c, 100:100 + N, 1] += np.round(2606 * np.sin(th + om * j)).astype(np.int32)
        xd = torch.from_numpy(x.astype(np.int16)).cuda()
        cors, demods = [], []
        for c in range(C_):
            g = S.FixedPatternCorrelator(N, 1)
            g.setPattern(pat)
            cors.append(g)
            d = S.DemodulatorOqpsk()
            d.setSyncPattern(np.ones(N, np.int8))
            demods.append(d)
        hits = S.corr_step_batched(cors, xd)
        found = [h[0] for h in hits]

        def batched():
            return S.demod_acquire_batched(demods, cors, found=found)

        def per_channel():
            est = []
            for c in range(C_):
                if not found[c]:
                    continue
                demods[c].setReference(cors[c])
                bs = cors[c].getRefBitSamples()
                si, sq = loop(bs[1:].view(np.uint32).reshape(-1), 1)
                f = np.float32(np.arctan2(float(sq), float(si)))
                demods[c].setInitialFrequency(float(np.float32(-1.0) * f))
                demods[c].reset()
                est.append(f)
            return est
        eb = batched()
        sb = [d.state() for d in demods]
        ep = per_channel()
        if [d.state() for d in demods] != sb or [v for v, k in zip(eb, found) if k] != ep:
            raise SystemExit(f"join {C_}: the join and the per-channel sequence disagree")
        steps = a.steps if C_ == 64 else max(a.steps // 10, 1)
        warm = a.warmup if C_ == 64 else max(a.warmup // 10, 1)
        ms = timed({"join": batched, "per_channel": per_channel, "join_again": batched,
                    "per_channel_again": per_channel}, warm, steps, lambda: None)
        r = {"channels": C_, "hits": int(sum(found)), "N": N, "warmup": warm, "steps": steps,
             "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
             "join_over_per_channel": round(min(ms["join"], ms["join_again"]) /
                                            min(ms["per_channel"], ms["per_channel_again"]), 4),
             "what": "both host code; the per-channel sequence goes through the Python face, 5 calls per channel"}
        out[str(C_)] = r
        print(json.dumps({f"join {C_}": r}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freqest_time.json"))
    ap.add_argument("--parts", default="sbj")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--today-rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import srcdsp_amd as S
    from srcdsp_amd.build import source_digest
    if not torch.cuda.is_available():
        raise SystemExit("freqest_time.py needs a GPU")
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0), "library_digest": source_digest(),
                "geometry_tile_vec_workgroups": list(S.FreqEstimator(1).geometry()),
                "protocol": "wall clock per call between device synchronisations; alternatives alternate within a "
                            "round, each timed twice; means of the timed rounds"})
    with tempfile.TemporaryDirectory() as tmp:
        loop = host_loop(tmp)
        if "s" in a.parts:
            res["stream"] = stream(S, torch, a, loop)
        if "b" in a.parts:
            res["bank"] = bank(S, torch, a)
        if "j" in a.parts:
            res["join"] = join(S, torch, a, loop)
    res.pop("command_line", None)
    for k in a.parts:  # parts may run as processes of their own, each under its own time limit
        res.setdefault("command_lines", {})[k] = (f"python scripts/freqest_time.py --parts {k} --warmup {a.warmup} "
                                                  f"--steps {a.steps} --today-rounds {a.today_rounds}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
