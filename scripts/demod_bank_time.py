"""Time srcdsp_demod_step_batched against the loop of srcdsp_demod_step over the
same handles.  One process per run, device-resident data, 100 warm-up rounds,
mean of 200 timed rounds.  A demodulator step returns its error to the host, so
the figure is wall-clock time per call (the call's own synchronise included),
taken between two device synchronisations.  Every round runs the batched call
and the loop on fresh clones of the same reset handles (cloned outside the timed
span); the batched call and the loop alternate, and the loop is timed twice per
round so its own run-to-run spread is on record.  Before timing, the two paths
must agree on soft bits, errors and states.  Needs a GPU (no fallback).

Shapes, P = 32, input uniform in +-16000: (a) 64 bursts x 16 384 samples;
(b) 8 x 16 384; (c) 1 x 16 384, the single step; (d) 64 frequency hypotheses on
one shared burst of 16 384; (e) 1024 x 4096, which fills 16 workgroups.

Results are merged into the output file shape by shape, so each shape can run
as a process of its own under its own time limit (and a long shape with fewer
rounds; every result records its own):
  for s in a b c d; do timeout -k 10 600 python scripts/demod_bank_time.py --shapes $s || break; done

--reference-host times the reference's own build (REF_DIR, g++ -O2, no
sanitiser, tests/cpp/demod_main.cpp) on shape (a) on one core of the machine
this runs on -- another host than the GPU box, and named as such in the file.

Usage: python scripts/demod_bank_time.py [--out profiles/demod_bank_time.json] [--shapes abcde]
       [--warmup 100] [--steps 200] [--reference-host]"""
import argparse
import copy
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

P = 32
SHAPES = {
    "a": dict(name="64 bursts x 16384", shared=False, n=1 << 14, C=64),
    "b": dict(name="8 bursts x 16384", shared=False, n=1 << 14, C=8),
    "c": dict(name="1 burst x 16384 (the single step)", shared=False, n=1 << 14, C=1),
    "d": dict(name="64 frequency hypotheses on one shared burst of 16384", shared=True, n=1 << 14, C=64),
    "e": dict(name="1024 bursts x 4096 (16 workgroups)", shared=False, n=1 << 12, C=1024),
}


def configure(d, rng, c, shared):
    bits = rng.integers(0, 2, P).astype(np.int8)
    ref = rng.integers(-16000, 16001, size=(P, 2)).astype(np.int16)
    word = (c - 32) * 3 if shared else int(rng.integers(-40, 41))
    return bits, ref, np.float32(word * np.pi / 4096), word


def measure(key, shape, warmup, steps):
    import torch
    import srcdsp_amd as S
    C, n, shared = shape["C"], shape["n"], shape["shared"]
    g = torch.Generator(device="cuda").manual_seed(ord(key))
    x = torch.randint(-16000, 16001, ((n, 2) if shared else (C, n, 2)), dtype=torch.int16, device="cuda", generator=g)
    rng = np.random.default_rng(ord(key))
    base = []
    shared_cfg = configure(None, rng, 0, True) if shared else None
    for c in range(C):
        bits, ref, f, word = configure(None, rng, c, shared)
        if shared:  # one burst: the same pattern and reference, another frequency word
            bits, ref = shared_cfg[0], shared_cfg[1]
        h = S.DemodulatorOqpsk()
        h.setSyncPattern(bits)
        h.setReference(ref)
        h.setInitialFrequency(float(f))
        h.reset()
        h.setInputShift(2)
        assert h.state()[7] == word
        base.append(h)
    rows = [x if shared else x[c] for c in range(C)]

    def clones():
        return [copy.copy(h) for h in base]

    def batched(hs):
        return S.demod_step_batched(hs, x)

    def loop(hs):
        return [hs[c].step(rows[c]) for c in range(C)]

    # the same step from the same state through both paths
    hb, hl = clones(), clones()
    soft, ns, errs = batched(hb)
    rl = loop(hl)
    for c in range(C):
        same = (ns[c] == n - P == len(rl[c][0]) and errs[c] == rl[c][1] and hb[c].state() == hl[c].state() and
                torch.equal(soft[c, :ns[c]], rl[c][0]))
        if not same:
            raise SystemExit(f"shape {key}: the batched call and the loop disagree on channel {c}")

    names = ("batched", "loop", "loop_again")
    fns = (batched, loop, loop)
    t = {k: [] for k in names}
    for i in range(warmup + steps):
        sets = [clones() for _ in names]
        for k, fn, hs in zip(names, fns, sets):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(hs)
            torch.cuda.synchronize()
            if i >= warmup:
                t[k].append(time.perf_counter() - t0)
    ms = {k: 1e3 * float(np.mean(v)) for k, v in t.items()}
    r = {
        "shape": shape["name"], "channels": C, "samples_per_channel": n, "P": P, "warmup": warmup, "steps": steps,
        "ms_per_call": {k: round(v, 5) for k, v in ms.items()},
        "samples_per_second": {k: round(C * n / (1e-3 * v)) for k, v in ms.items()},
        "loop_spread_ms": round(abs(ms["loop"] - ms["loop_again"]), 5),
        "batched_over_loop": round(ms["batched"] / min(ms["loop"], ms["loop_again"]), 4),
    }
    print(json.dumps(r), flush=True)
    return r


def reference_host(runs=5):
    """The reference's own build on this machine's CPU, one core: 64 bursts x
    16 384 samples, P = 32, one object per burst (shape (a))."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_demod_golden as G
    ref_dir = os.environ.get("REF_DIR", G.REF)
    rng = np.random.default_rng(ord("a"))
    C, n = 64, 1 << 14
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "demod_ref")
        subprocess.run(["g++", "-std=gnu++11", "-O2", "-I", ref_dir, G.SRC, os.path.join(ref_dir, "demodulators.cpp"),
                        "-o", exe], check=True)
        args = []
        for c in range(C):
            bits, ref, f, _ = configure(None, rng, c, False)
            blob = G.case_bin({"bits": bits, "ref": ref, "shift": 2, "freq": f, "reset_before": -1, "chunks": [n],
                               "x": rng.integers(-16000, 16001, size=(n, 2)).astype(np.int16)})
            with open(os.path.join(d, f"{c}.case"), "wb") as fh:
                fh.write(blob)
            args += [f"{c}.case", f"{c}.out"]
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            subprocess.run([exe] + args, cwd=d, check=True)
            ts.append(time.perf_counter() - t0)
    cpu = ""
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "")
    except OSError:
        pass
    ms = 1e3 * min(ts)
    return {"what": "the reference's DemodulatorOqpsk<int16_t> (g++ -O2, no sanitiser), one process on one core, "
                    "64 objects x one step() of 16384 samples; the 64 constructors (each builds both tables), "
                    "case files read and outputs written are included",
            "host": "another host than the GPU box: " + (cpu or platform.processor() or platform.machine()),
            "runs": runs, "ms_min": round(ms, 3), "ms_mean": round(1e3 * float(np.mean(ts)), 3),
            "samples_per_second": round(C * n / (1e-3 * ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demod_bank_time.json"))
    ap.add_argument("--shapes", default="abcde")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reference-host", action="store_true")
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.reference_host:
        res["reference_on_a_host_core"] = reference_host()
        print(json.dumps(res["reference_on_a_host_core"]), flush=True)
    else:
        import torch
        from srcdsp_amd.build import source_digest
        if not torch.cuda.is_available():
            raise SystemExit("demod_bank_time.py needs a GPU")
        res.update({"device": torch.cuda.get_device_name(0), "library_digest": source_digest(),
                    "protocol": "wall clock per call between device synchronisations, fresh clones of reset handles "
                                "per round; batched, loop, loop alternate per round; means"})
        res.setdefault("results", {})
        res.setdefault("command_lines", {})
        for k in a.shapes:
            res["results"][k] = measure(k, SHAPES[k], a.warmup, a.steps)
            res["command_lines"][k] = (f"python scripts/demod_bank_time.py --shapes {k} --warmup {a.warmup} "
                                       f"--steps {a.steps}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
