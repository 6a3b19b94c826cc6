"""Child process of tests/test_gpu_corr_all.py: srcdsp_corr_step_all of the
always-exact correlator build (tests/_build/libsrcdsp_hip_corr_exact.so:
corr.hip, corr_bank.hip and corr_all.hip with -DSRCDSP_CORR_ALWAYS_EXACT) with
NO product library in the process -- the package is pointed at that build
through SRCDSP_HIP_LIB, so every C-ABI call and kernel launch is that build's own.

  python tests/corr_all_exact_child.py EXACT_SO OUT.json

Runs the back-to-back and straddle rows of corr_all_model.cases(), each call
checked against the oracle loop.  OUT.json: whether the product library got
mapped (it must not), the build flags a kernel of the loaded library reports,
the detections per row and the library's (kernel, loop) counters."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    exact, out = sys.argv[1], sys.argv[2]
    os.environ["SRCDSP_HIP_LIB"] = exact  # read by srcdsp_amd._capi at import
    import pyoracle
    import srcdsp_amd as S
    import corr_all_model as M
    import test_gpu_corr_all as T
    f = C.c_uint(99)
    assert S.lib().srcdsp_build_flags(C.byref(f)) == 0
    O = {"fma": pyoracle.Oracle(1)}
    events, calls = {}, 0
    for name, case in M.cases().items():
        if name.startswith("b2b_") or name == "straddle":
            got = T.run_case(S, O, case)
            events[name] = [c[1] for c in got]
            calls += len(got)
    product = os.path.join(ROOT, "srcdsp_amd", "lib", "libsrcdsp_hip.so")
    with open("/proc/self/maps") as m:
        mapped = product in m.read()
    with open(out, "w") as fh:
        json.dump({"build_flags": int(f.value), "product_mapped": mapped, "events": events, "calls": calls,
                   "stats": list(S.corr_all_stats())}, fh)


if __name__ == "__main__":
    main()
