"""tests/demod_model.py, the plain-Python restatement of the reference's
DemodulatorOqpsk<int16_t>::step, against the goldens recorded from the
reference itself (tests/golden/gen_demod_golden.py): every case bit for bit,
and the two lookup tables.  CPU only."""
import numpy as np
import pytest

import demod_model as M

MAN, ARR = M.load_golden()


def test_model_tables_equal_the_reference_tables():
    sine, phase = M.tables()
    assert np.array_equal(sine, ARR["sine"]) and np.array_equal(phase, ARR["phase"])
    assert MAN["tables"] == {"sine": 8192, "phase": 128 * 128}


def test_manifest_holds_the_cases_around_the_tile():
    T = MAN["tile"]
    keys = {c["key"] for c in MAN["cases"]}
    for n in (1, 31, 32, 33, T - 1, T, T + 1, 2 * T + 5):
        assert f"n{n}" in keys
    for P in (2, 16, T + 3):
        assert {f"p{P}", f"p{P}_first"} <= keys
    assert {"shift0", "shift3", "shift8", "amp100", "amp16000", "amp32767", "word0", "word13", "word-13", "word4096",
            "word-4096", "chain", "reset", "locked"} <= keys


@pytest.mark.parametrize("key", [c["key"] for c in MAN["cases"]])
def test_model_equals_the_reference(key):
    case = next(c for c in MAN["cases"] if c["key"] == key)
    m = M.golden_case_model(case, ARR)
    assert m.freq == case["word"]
    x, pos, spos = ARR[key + "_x"], 0, 0
    for i, n in enumerate(case["chunks"]):
        if i == case["reset_before"]:
            m.reset()
        soft, err = m.step(x[pos:pos + n])
        pos += n
        ns = case["soft_sizes"][i]
        assert len(soft) == ns
        assert np.array_equal(soft, ARR[key + "_soft"][spos:spos + ns]), (key, i)
        spos += ns
        assert err == ARR[key + "_error"][i], (key, i)
        assert m.measured_frequency().tobytes() == ARR[key + "_mfreq"][i].tobytes(), (key, i)


def test_short_call_measures_frequency_zero():
    """numIn < 32: freqComputationStart goes negative through int and then
    unsigned (demodulators.cpp:181, :264), so nothing is accumulated."""
    case = next(c for c in MAN["cases"] if c["key"] == "chain")
    assert case["chunks"][2] < 32
    assert ARR["chain_mfreq"][2] == 0.0 and ARR["chain_mfreq"][0] != 0.0


def test_locked_burst_decodes_the_transmitted_bits():
    soft, tx = ARR["locked_soft"], ARR["locked_tx_bits"]
    assert len(soft) == len(tx) and np.array_equal(soft > 0, tx > 0)
    assert np.abs(soft).max() < 127  # the shift keeps the soft bits out of saturation
    # the carrier offset, 0.01 rad/sample, is what the loop measures
    assert abs(float(ARR["locked_mfreq"][0]) - 0.01) < 2 * np.pi / 4096
