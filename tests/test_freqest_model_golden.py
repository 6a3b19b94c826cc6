"""tests/freqest_model.py, the plain-Python restatement of the reference's
estimateFreq<int16_t, L>, against the goldens recorded from the reference
itself (tests/golden/gen_freqest_golden.py): every case bit for bit.  CPU only."""
import numpy as np
import pytest

import freqest_model as M

MAN, ARR = M.load_golden()
CASES = {c["key"]: c for c in MAN["cases"]}


def test_manifest_holds_the_case_matrix():
    for L in (1, 2, 3, 4, 8, 32):
        for kind in ("noise", "full", "tone"):
            for n in (0, 1, L, L + 1, 33, 257, 1000, 4097):
                assert f"{kind}_L{L}_n{n}" in CASES
    assert int(np.abs(ARR["full"]).min()) == 32767 and int(np.abs(ARR["noise"]).max()) > 32700
    for name in ARR.files:  # the reference is undefined at -32768 pairs: no golden holds one
        assert int(ARR[name].min()) > -32768, name


@pytest.mark.parametrize("key", list(CASES))
def test_model_equals_the_reference(key):
    c = CASES[key]
    f, (si, sq), exact = M.estimate(ARR[c["input"]][:c["n"]], c["L"])
    assert exact  # (n - L) * T < 4097 * 2^31 < 2^53
    assert M.bits(f) == c["bits"], (key, f)
    if c["n"] <= c["L"]:
        assert (si, sq) == (0, 0) and c["bits"] == 0  # +0.0f


def test_tone_estimates_are_minus_the_tone_frequency():
    """x[i] conj(x[i+L]) of e^{+jwn} has the phase -wL: the estimator returns -w."""
    for c in MAN["cases"]:
        if c["kind"] == "tone" and c["n"] >= 257:
            f = np.array([c["bits"]], np.uint32).view(np.float32)[0]
            assert abs(float(f) + c["omega"]) < 2e-3, c["key"]


def test_model_wraps_the_overflowing_term():
    x = np.full((3, 2), -32768, np.int16)
    ti, tq = M.terms(x, 1)
    assert ti.tolist() == [-(1 << 31)] * 2 and tq.tolist() == [0, 0]
    f, sums, exact = M.estimate(x, 1)
    assert sums == (-(1 << 32), 0) and exact and f == np.float32(np.pi)


def test_exact_flag_follows_the_bound():
    full = np.full(((1 << 22) + 4098, 2), 32767, np.int16)
    T = 2 * 32767 ** 2
    assert (1 << 22) * T < 1 << 53 <= ((1 << 22) + 4097) * T
    f, sums, exact = M.estimate(full[:(1 << 22) + 1], 1)
    assert exact and sums == ((1 << 22) * T, 0)
    f, sums, exact = M.estimate(full, 1)
    assert not exact and sums == (((1 << 22) + 4097) * T, 0)
