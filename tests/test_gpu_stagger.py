"""The Q-rail stagger on the GPU (srcdsp_stagger_step, _step_host on a handle
the device holds, _step_batched) against the numpy model: outputs and the carry
bit for bit, for n below D, around the 1024-sample workgroup tile and across
several workgroups, aligned and unaligned buffers, streams in chunks, banks
against the loop, and refusals that change nothing."""
import copy

import numpy as np
import pytest

import stagger_model as G

pytestmark = pytest.mark.gpu

TILE = 1024


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def samples(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, 2)).astype(np.int16)


def primed(S, D, seed):
    """A stagger whose carry the device holds, and the model of the same."""
    g, m = S.QStagger(D), G.StaggerModel(D)
    x = samples(D + 5, seed)
    assert np.array_equal(g.step(dev(x)).cpu().numpy(), m.step(x))
    return g, m


def test_geometry(S):
    assert S.stagger_geometry() == (TILE, 64)


@pytest.mark.parametrize("D", [1, 2, 4, 7, 64])
def test_step_equals_the_model(S, D):
    import torch
    g, m = primed(S, D, D)
    # below D, around D, around one tile, several workgroups with a partial last one
    for k, n in enumerate((1, D - 1, D, D + 1, 3, TILE - 1, TILE, TILE + 1, 5 * TILE + 13)):
        if n == 0:
            continue
        x = samples(n, 100 * D + k)
        out = torch.full((n + 4, 2), 77, dtype=torch.int16, device="cuda")
        g.step(dev(x), out[:n])
        y = out.cpu().numpy()
        assert np.array_equal(y[:n], m.step(x)), n
        assert (y[n:] == 77).all()
        assert g.state().tolist() == m.carry.tolist(), n


def test_unaligned_buffers_and_host_buffers(S):
    """Buffers off 16-byte alignment take the kernel's scalar form; a handle
    the device holds stages host buffers over."""
    g, m = primed(S, 4, 9)
    x = samples(2 * TILE + 8, 10)
    xd, out = dev(x), dev(np.zeros((2 * TILE + 16, 2), np.int16))
    for lo_in, lo_out in ((1, 0), (0, 3), (1, 1), (2, 5)):
        n = 2 * TILE + 3
        g.step(xd[lo_in:lo_in + n], out[lo_out:lo_out + n])
        assert np.array_equal(out[lo_out:lo_out + n].cpu().numpy(), m.step(x[lo_in:lo_in + n])), (lo_in, lo_out)
        assert g.state().tolist() == m.carry.tolist()
    y = g.step(x[:TILE + 5])  # numpy in: srcdsp_stagger_step_host
    assert np.array_equal(y, m.step(x[:TILE + 5])) and g.state().tolist() == m.carry.tolist()
    assert np.array_equal(g.step(dev(x[:7])).cpu().numpy(), m.step(x[:7]))


def test_copy_reset_and_chunks(S):
    g, m = primed(S, 8, 11)
    x = samples(3 * TILE, 12)
    whole = copy.copy(g).step(dev(x)).cpu().numpy()
    assert np.array_equal(whole, m.copy().step(x))
    c = copy.copy(g)
    parts = [c.step(dev(x[a:b])).cpu().numpy() for a, b in ((0, 3), (3, 4), (4, TILE + 4), (TILE + 4, 3 * TILE))]
    assert np.array_equal(np.concatenate(parts), whole)
    assert c.state().tolist() == x[-8:, 1].tolist()  # the last D imaginary halves seen
    assert g.state().tolist() == m.carry.tolist()  # the copies left the original alone
    g.reset()
    m.reset()
    assert g.state().tolist() == [0] * 8
    assert np.array_equal(g.step(dev(x[:100])).cpu().numpy(), m.step(x[:100]))


@pytest.mark.parametrize("shared", [True, False], ids=["shared_in", "in_per_row"])
@pytest.mark.parametrize("rows", [3, 65])
def test_bank_equals_the_loop(S, rows, shared):
    """65 rows cross kMaxBatch = 64; every row has its own carry.  Row strides
    of whole granules, then odd ones (the scalar form)."""
    import torch
    D = 4
    pairs = [primed(S, D, 20 + r) for r in range(rows)]
    for n, pad in ((TILE + 12, 4), (TILE + 13, 0)):
        x = samples(rows * n, n).reshape(rows, n, 2)
        xd = dev(x[0]) if shared else dev(x)
        out = torch.full((rows, n + pad, 2), 77, dtype=torch.int16, device="cuda")
        S.stagger_step_batched([g for g, _ in pairs], xd, out)
        y = out.cpu().numpy()
        assert (y[:, n:] == 77).all()
        for r, (g, m) in enumerate(pairs):
            assert np.array_equal(y[r, :n], m.step(x[0 if shared else r])), (n, r)
            assert g.state().tolist() == m.carry.tolist()


def test_refusals_change_nothing(S):
    import torch
    from srcdsp_amd import _capi as A
    g, m = primed(S, 4, 30)
    h, _ = primed(S, 5, 31)
    buf = torch.zeros((64, 2), dtype=torch.int16, device="cuda")

    def refused(code, fn):
        with pytest.raises(S.SrcdspError) as e:
            fn()
        assert e.value.code == code

    refused(A.ERR_ARG, lambda: g.step(buf[:16], buf[:16]))       # in place
    refused(A.ERR_ARG, lambda: g.step(buf[:16], buf[8:24]))      # out overlaps the input's tail
    refused(A.ERR_ARG, lambda: g.step(buf[8:24], buf[:16]))
    out = torch.zeros((2, 16, 2), dtype=torch.int16, device="cuda")
    refused(A.ERR_ARG, lambda: S.stagger_step_batched([g, g], buf[:16], out))   # listed twice
    refused(A.ERR_ARG, lambda: S.stagger_step_batched([g, h], buf[:16], out))   # D differs
    refused(A.ERR_SIZE, lambda: S.stagger_step_batched([g, copy.copy(g)], buf[:17], out))  # out_stride short
    assert g.state().tolist() == m.carry.tolist()
    x = samples(16, 32)
    assert np.array_equal(g.step(dev(x)).cpu().numpy(), m.step(x))
