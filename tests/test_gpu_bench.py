"""bench.py's plain run on the GPU, in this process and at a small size: the
line's headline fields, no leg beside them, and --dump-outputs holding the
last timed step's output of the HIP decimator bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

N = (1 << 16) + 4 * 37  # several blocks, not a multiple of the kernel's tile


def _run(capsys, *args):
    bench.main(["--gpus", "1", "--samples", str(N), *args])
    return json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])


def test_plain_run_line_and_dumped_outputs(S, O, tmp_path, capsys):
    from srcdsp_amd.design import hamming_sinc
    d = str(tmp_path / "out")
    line = _run(capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", d)
    assert line["metric"] == bench.METRIC and line["unit"] == "Msamples/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 2
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # the two say the same thing; ms_per_step is rounded to 1e-4 ms of a step no shorter than ~5 us
    assert abs(line["value"] - N / line["ms_per_step"] / 1e3) <= 0.02 * line["value"]
    for leg in ("parity", "configs2_share", "cpu_baseline", "cpu_baseline_allcores", "cpu_baseline_O0",
                "pcie_inclusive"):
        assert leg not in line, leg
    assert line["dumped_outputs"] == {"y.npy": {"rows": N // 4, "of": N // 4, "dtype": "float32"}}
    y = np.load(os.path.join(d, "y.npy"))
    x = O["fma"].gen_cf32(bench.SEED, 0, 0, N)
    f = O["fma"].decim(0, 4, hamming_sinc(127))
    for _ in range(5):  # 2 warm-up + 3 timed steps continue one stream
        want = f.step(x)
    assert y.dtype == np.float32 and y.shape == (N // 4, 2)
    assert np.array_equal(y.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1))


def test_mixdecim_dump_is_exact_int16_and_repeats(S, tmp_path, capsys):
    """An int16 output goes out as float32 without loss, and a second run with
    the same arguments writes the same bytes (seeded input)."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        _run(capsys, "--workload", "mixdecim", "--steps", "2", "--warmup", "1", "--dump-outputs", d)
    ya, yb = (np.load(os.path.join(d, "y.npy")) for d in (a, b))
    assert ya.dtype == np.float32 and ya.shape == (N // 4, 2) and np.array_equal(ya, yb)
    assert np.array_equal(ya, ya.astype(np.int16)) and np.any(ya != 0)


def test_dump_sampled_on_the_device_within_a_small_budget(S, O, tmp_path, capsys, monkeypatch):
    """An output above the budget is sampled on the device: the rows written
    are the oracle's at the documented indices, one per stratum [i*n // k,
    (i+1)*n // k), the last rows of the output among them."""
    from srcdsp_amd.design import hamming_sinc
    n, k = N // 4, 4096
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", k * 8)
    d = str(tmp_path / "out")
    line = _run(capsys, "--steps", "2", "--warmup", "1", "--dump-outputs", d)
    assert line["dumped_outputs"] == {"y.npy": {"rows": k, "of": n, "dtype": "float32"}}
    x = O["fma"].gen_cf32(bench.SEED, 0, 0, N)
    f = O["fma"].decim(0, 4, hamming_sinc(127))
    for _ in range(3):
        want = f.step(x)
    lo = np.arange(k + 1, dtype=np.int64) * n // k
    idx = lo[:-1] + np.random.default_rng(bench.SEED).integers(0, np.diff(lo))
    assert idx[-1] >= n - 5 and np.all(np.diff(idx) > 0)
    y = np.load(os.path.join(d, "y.npy"))
    assert np.array_equal(y.view(np.uint32).reshape(-1), want[idx].view(np.uint32).reshape(-1))


def test_fir_input_is_seeded_and_its_dump_is_the_operator_output(S, tmp_path, capsys):
    """--workload fir: the input comes from a seeded device generator, so two
    runs dump the same bytes, and they are FilterFir's third chained step over
    that input (1 warm-up + 2 timed)."""
    import torch
    from srcdsp_amd.design import hamming_sinc
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        _run(capsys, "--workload", "fir", "--steps", "2", "--warmup", "1", "--dump-outputs", d)
    ya, yb = (np.load(os.path.join(d, "y.npy")) for d in (a, b))
    assert ya.dtype == np.float32 and ya.shape == (N, 2)
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
    g = torch.Generator(device="cuda")
    g.manual_seed(bench.SEED)
    x = torch.randint(-2048, 2048, (N,), device="cuda", generator=g).float()
    assert x.min() < -1000 and x.max() > 1000
    f = S.FilterFir(hamming_sinc(31, 0.2), "float", "complex<float>", "float", "float", fp="fma")
    y = torch.empty(N, dtype=torch.complex64, device="cuda")
    for _ in range(3):
        f.step(x, y)
    want = torch.view_as_real(y).cpu().numpy()
    assert np.array_equal(ya.view(np.uint32), want.view(np.uint32))


def test_corr_dump_is_the_detection(S, O, tmp_path, capsys):
    """--workload corr: detection.npy is (found, index) of the last step, the
    line's `detection`, and the oracle's over the same buffer."""
    from srcdsp_amd.design import qpsk_pattern
    L = 1 << 17
    d = str(tmp_path / "out")
    bench.main(["--gpus", "1", "--workload", "corr", "--samples", str(L), "--steps", "2", "--warmup", "1",
                "--dump-outputs", d])
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    det = np.load(os.path.join(d, "detection.npy"))
    assert det.dtype == np.float64 and det.shape == (2, 1)
    p = qpsk_pattern(1024, 500, seed=2)
    x = np.random.default_rng(0).integers(-125, 126, size=(L, 2)).astype(np.int32)
    x[(3 * L) // 4:(3 * L) // 4 + 1024] += 2 * p
    r = O["fma"].corr(1024, 1)
    r.set_pattern(p)
    found, idx = r.step(np.clip(x, -32768, 32767).astype(np.int16))
    assert found and [bool(det[0, 0]), int(det[1, 0])] == [found, idx] == [bool(line["detection"][0]), line["detection"][1]]
