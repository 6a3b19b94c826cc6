"""Child process of tests/test_gpu_corr_bank.py: srcdsp_corr_step_batched of the
always-exact correlator build (tests/_build/libsrcdsp_hip_corr_exact.so:
corr.hip and corr_bank.hip with -DSRCDSP_CORR_ALWAYS_EXACT) with NO product
library in the process -- the package is pointed at that build through
SRCDSP_HIP_LIB, so every C-ABI call and kernel launch is that build's own.

  python tests/corr_bank_exact_child.py EXACT_SO OUT.json

Runs case 1's N = 64, C = 8 signal (test_gpu_corr_bank.case1_signal), stepping
on after every detection, each step checked against the oracle.  OUT.json:
whether the product library got mapped (it must not), the build flags a kernel
of the loaded library reports, the detections per channel, the number of
batched calls and the library's (bank, loop) counters."""
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
    import test_gpu_corr_bank as T
    f = C.c_uint(99)
    assert S.lib().srcdsp_build_flags(C.byref(f)) == 0
    O = {"fma": pyoracle.Oracle(1)}
    ps, x, _ = T.case1_signal(64, 8)
    cors, refs = T.make(S, O, ps, 64)
    events, calls = T.run_stepping(S, cors, refs, x)
    product = os.path.join(ROOT, "srcdsp_amd", "lib", "libsrcdsp_hip.so")
    with open("/proc/self/maps") as m:
        mapped = product in m.read()
    with open(out, "w") as fh:
        json.dump({"build_flags": int(f.value), "product_mapped": mapped, "events": events, "calls": calls,
                   "stats": list(S.corr_batched_stats())}, fh)


if __name__ == "__main__":
    main()
