"""The Python model of the symbol mappers (tests/mapper_model.py) equals every
golden recorded from the reference's modulators.h, and the transmit-chain
goldens equal mapper model -> oracle interpolator -> oracle mixer."""
import numpy as np
import pytest

import mapper_model as M

MAN, ARR = M.load_golden()


def test_golden_set_is_what_the_suite_expects():
    assert MAN["bit_bytes"] == [0, 1, 2, 128, 255]
    keys = {c["key"] for c in MAN["cases"]}
    for name, lens in (("sdpsk", (0, 1, 2, 3, 255, 256, 257)), ("qpsk", (0, 2, 256))):
        assert {f"{name}_n{n}" for n in lens} <= keys
        assert {f"{name}_{k}" for k in ("chunks", "reset", "copy", "empty_mid")} <= keys
    assert len(MAN["chains"]) == 4
    for c in MAN["cases"]:  # every byte value of the set occurs, so "non-zero is a one" is exercised
        if sum(c["calls"]) >= 255:
            assert set(np.unique(ARR[c["key"] + "_bits"])) == set(MAN["bit_bytes"])


@pytest.mark.parametrize("case", MAN["cases"], ids=[c["key"] for c in MAN["cases"]])
def test_model_equals_the_reference(case):
    m = M.MapperModel(case["kind"])
    for i, (bits, sym, state) in enumerate(M.golden_calls(case, ARR)):
        if i == case["reset_before"]:
            m.reset()
        before = m.state
        y = m.step(bits)
        assert np.array_equal(y, sym) and m.state == state
        y2, s2 = M.step_loop(case["kind"], before, bits)
        assert np.array_equal(y2, sym) and s2 == state
    assert np.array_equal(np.concatenate(M.parse_out(ARR[case["key"] + "_out"].tobytes(), len(case["calls"]))),
                          ARR[case["key"] + "_sym"])


def test_nonzero_bytes_are_ones():
    for kind in (M.SDPSK, M.QPSK):
        ones = M.MapperModel(kind).step(np.ones(64, np.uint8))
        for v in (2, 128, 255):
            assert np.array_equal(M.MapperModel(kind).step(np.full(64, v, np.uint8)), ones)


@pytest.mark.parametrize("chain", MAN["chains"], ids=[c["key"] for c in MAN["chains"]])
def test_chain_golden_equals_model_and_oracle(chain):
    import pyoracle
    o = pyoracle.Oracle()
    k = chain["key"]
    m = M.MapperModel(chain["kind"])
    up = o.up(0, chain["L"], ARR[k + "_taps"])
    mixer = o.mixer(chain["N"])
    mixer.set_frequency(chain["freq"])
    bits, pos, ys = ARR[k + "_bits"], 0, []
    for n, flush in zip(chain["calls"], chain["flush"]):
        ys.append(mixer.step(up.step(m.step(bits[pos:pos + n]), flush=flush)))
        pos += n
    assert np.array_equal(np.concatenate(ys).reshape(-1, 2), ARR[k + "_out"])
