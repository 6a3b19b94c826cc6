"""Record the offset-QPSK transmit chain goldens (oqpsk_golden.npz / .json) from
the reference build: the symbols of the mapper model (pinned to the reference's
mappers by tests/test_mapper_model_golden.py) through the reference's own
FilterUpsamplingFir::step and Mixer::step (pyoracle.Reference, compiled from
the reference tree), with the Q-rail delay between them done here in numpy --
the reference leaves that delay to the application, so there is no reference
code for it to record.

Run where the reference build exists (oracle/_ref): python tests/golden/gen_oqpsk_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BIT_BYTES = np.array([0, 1, 2, 128, 255], np.uint8)  # a one is any non-zero byte


def main():
    import mapper_model as M
    import pyoracle
    ref = pyoracle.Reference("strict")
    rng = np.random.default_rng(20262)
    arrays, chains = {}, []
    for kind, name in ((M.SDPSK, "sdpsk"), (M.QPSK, "qpsk")):
        for L, ntaps, D, freq, nsym in ((4, 16, 2, 0.1137, (150, 173)), (8, 32, 4, -0.3021, (97, 204))):
            for flush in ((False, False), (False, True)):
                key = f"oqpsk_{name}_L{L}_{'flush' if flush[1] else 'plain'}"
                taps = rng.integers(-2000, 2001, ntaps).astype(np.int32)
                per = 2 if kind == M.QPSK else 1
                calls = [n * per for n in nsym]
                bits = rng.choice(BIT_BYTES, sum(calls))
                mapper, up, mixer = M.MapperModel(kind), ref.up(0, L, taps), ref.mixer(4096)
                mixer.reset(freq)
                carry = np.zeros(D, np.int16)
                pos, ys = 0, []
                for n, fl in zip(calls, flush):
                    y = np.asarray(up.step(mapper.step(bits[pos:pos + n]), fl)).reshape(-1, 2).copy()
                    pos += n
                    v = np.concatenate([carry, y[:, 1]])  # the delay line: D samples on the imaginary rail
                    y[:, 1] = v[:len(y)]
                    carry = v[len(y):len(y) + D]
                    ys.append(np.asarray(mixer.step(y)).reshape(-1, 2))
                arrays[key + "_bits"], arrays[key + "_taps"] = bits, taps
                arrays[key + "_out"] = np.concatenate(ys).astype(np.int16)
                arrays[key + "_carry"] = carry.astype(np.int16)
                chains.append({"key": key, "kind": kind, "L": L, "D": D, "N": 4096, "freq": freq, "ntaps": ntaps,
                               "calls": calls, "flush": list(flush), "mapper_state": mapper.state,
                               "mixer_phase": int(mixer.state()[0])})
                print(chains[-1], arrays[key + "_out"].shape)
    np.savez_compressed(os.path.join(HERE, "oqpsk_golden.npz"), **arrays)
    with open(os.path.join(HERE, "oqpsk_golden.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_oqpsk_golden.py",
                   "source": "reference upsampling_filters.h and mixers.h through pyoracle.Reference('strict'); "
                             "symbols from tests/mapper_model.py; the Q-rail delay in numpy",
                   "bit_bytes": [int(b) for b in BIT_BYTES], "chains": chains}, f, indent=1)


if __name__ == "__main__":
    main()
