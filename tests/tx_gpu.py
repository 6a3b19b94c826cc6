"""The device side of the transmit-chain tests: the handles of one chain of a
fused family (upmix, modulate, modulate_offset) behind the interface of
tx_chain_model.TxChain, so that a test steps both with the same calls.  The
fused call, the separate operators on the same handles, the family's path
counters and its bank entry point (through the C ABI: any strides, a null
input of no bits or samples)."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

import mapper_model as M
from tx_chain_model import MODULATE, MODULATE_OFFSET, UPMIX

UP_T = {0: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int32_t"),
        1: ("complex<int16_t>", "complex<int16_t>", "complex<int32_t>", "int16_t")}
GUARD, GUARD_VALUE = 24, 77
BIT_BYTES = np.array([0, 1, 2, 128, 255], np.uint8)  # a bit is a one when its byte is non-zero


def dev(x):
    """An allocation of its own: 16-byte aligned."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def dev_off(x):
    """The same values in a view one element (a byte of bits, a sample of 4
    bytes) off 16-byte alignment."""
    import torch
    x = np.ascontiguousarray(x)
    buf = torch.empty((len(x) + 1,) + x.shape[1:], dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda()
    v = buf[1:]
    assert v.data_ptr() % 16 != 0
    return v


class GpuChain:
    def __init__(self, S, family, L, taps, N=4096, freq=0.0, kind=None, D=None, variant=0, mapper_state=0):
        self.S, self.family, self.kind, self.L = S, family, kind, L
        self.mapper = self.stagger = None
        if family != UPMIX:
            self.mapper = (S.SymbolMapperQpsk if kind == M.QPSK else S.SymbolMapperSdpsk)()
            self.mapper.setState(mapper_state)
        c = np.asarray(taps)
        self.up = S.FilterUpsamplingFir(c.astype(np.int16) if variant == 1 else c, L, *UP_T[variant])
        if family == MODULATE_OFFSET:
            self.stagger = S.QStagger(D)
        self.mixer = S.Mixer(N)
        self.mixer.reset(freq)

    def copy(self):
        c = copy.copy(self)
        c.up, c.mixer = copy.copy(self.up), copy.copy(self.mixer)
        c.mapper = copy.copy(self.mapper) if self.mapper else None
        c.stagger = copy.copy(self.stagger) if self.stagger else None
        return c

    def stats(self):
        """(fused, pair or sequence, bank, loop) calls of the family so far."""
        return getattr(self.S, self.family + "_stats")()

    def n_out(self, n, flush=False):
        n_sym = self.mapper.n_out(n) if self.mapper else n
        return self.L * (n_sym + (self.up.getLength() // self.L if flush else 0))

    def guarded(self, n_out):
        import torch
        return torch.full((n_out + GUARD, 2), GUARD_VALUE, dtype=torch.int16, device="cuda")

    def fused(self, xd, flush=False, iterator=False, out=None):
        S = self.S
        if self.family == UPMIX:
            return S.UpsamplerMixerChain(self.up, self.mixer).step(xd, out, flush, iterator)
        if self.family == MODULATE:
            return S.ModulatorChain(self.mapper, self.up, self.mixer).step(xd, out, flush, iterator)
        return S.OffsetModulatorChain(self.mapper, self.up, self.stagger, self.mixer).step(xd, out, flush, iterator)

    def separate(self, xd, flush=False, iterator=False):
        """The operators one after the other on the same handles."""
        y = self.up.step(self.mapper.step(xd) if self.mapper else xd, None, flush, iterator)
        return self.mixer.step(self.stagger.step(y) if self.stagger else y)

    def state(self) -> dict:
        s = {"mixer": tuple(self.mixer.state()[:2])}
        if self.mapper:
            s["mapper"] = self.mapper.state()
        if self.stagger:
            s["carry"] = self.stagger.state().tolist()
        return s

    def set_frequency(self, f):
        self.mixer.setFrequency(f)

    def adjust_frequency(self, f):
        self.mixer.adjustFrequency(f)

    def reset_mapper(self):
        self.mapper.reset()

    def set_mapper_state(self, s):
        self.mapper.setState(s)

    def reset_stagger(self):
        self.stagger.reset()

    def reset_up(self):
        self.up.reset()


def stats_delta(ch: GpuChain, fn):
    s0 = ch.stats()
    r = fn()
    return r, tuple(b - a for a, b in zip(s0, ch.stats()))


def bank_step(chains, xd, in_stride, out, n, flush):
    """srcdsp_<family>_step_batched on the chains' handles.  xd: a device
    tensor or None (n = 0); in_stride: bits or samples between rows, 0 for one
    shared input; out: int16 [rows, out_stride, 2]."""
    from srcdsp_amd import _capi as A
    from srcdsp_amd.operators import _handles, _ptr, _stream
    family = chains[0].family
    hs = [_handles([c.mapper for c in chains])] if family != UPMIX else []
    hs.append(_handles([c.up for c in chains]))
    if family == MODULATE_OFFSET:
        hs.append(_handles([c.stagger for c in chains]))
    hs.append(_handles([c.mixer for c in chains]))
    A.call(f"srcdsp_{family}_step_batched", *hs, len(chains), C.c_void_p(xd.data_ptr() if xd is not None else None),
           in_stride, _ptr(out), out.shape[1], n, int(flush), _stream(out))
