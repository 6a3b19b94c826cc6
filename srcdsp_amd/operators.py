"""Host-side mirror of SrcDsp's hot-path operator classes over libsrcdsp_hip.so.

Each class keeps the reference's name, constructor arguments, template
parameters (as constructor arguments) and ``step()`` contract; the compute runs
in the HIP kernels behind the C ABI (include/srcdsp_hip.h).  Buffers may be

* numpy arrays (host) -- staged through pinned memory, synchronous, like the
  reference's std::vector calls;
* torch tensors on the GPU -- device-resident, asynchronous on torch's current
  stream (the benchmark path).

Sample layouts match std::complex<T> in memory: complex<float> -> complex64[n]
(or float32[n,2]); complex<int16_t> -> int16[n,2]; complex<int32_t> -> int32[n,2];
float -> float32[n]; int16_t -> int16[n].

Like the reference, ``step(in, out)`` requires ``out`` pre-sized; ``step(in)``
allocates and returns it.  Size violations the reference asserts on raise
``SrcdspError`` (code SRCDSP_ERR_SIZE).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as A

_ALIASES = {
    "cf32": "cf32", "complex<float>": "cf32", "std::complex<float>": "cf32",
    "ci16": "ci16", "complex<int16_t>": "ci16", "std::complex<int16_t>": "ci16", "complex<short>": "ci16",
    "ci32": "ci32", "complex<int32_t>": "ci32", "std::complex<int32_t>": "ci32", "complex<int>": "ci32",
    "f32": "f32", "float": "f32",
    "i16": "i16", "int16_t": "i16", "short": "i16",
    "i32": "i32", "int32_t": "i32", "int": "i32",
}
_NP = {"cf32": np.complex64, "ci16": np.int16, "ci32": np.int32, "f32": np.float32, "i16": np.int16,
       "i32": np.int32}
_BYTES = {"cf32": 8, "ci16": 4, "ci32": 8, "f32": 4, "i16": 2, "i32": 4}


def _kind(t: str) -> str:
    try:
        return _ALIASES[t.replace(" ", "")]
    except KeyError:
        raise TypeError(f"unknown sample/coefficient type {t!r}") from None


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _nsamples(x, kind: str) -> int:
    if _is_device(x):
        nb = x.numel() * x.element_size()
    else:
        nb = np.asarray(x).nbytes
    return nb // _BYTES[kind]


def _host(x, kind: str) -> np.ndarray:
    a = np.ascontiguousarray(x)
    if kind in ("ci16", "ci32"):
        a = np.ascontiguousarray(a, _NP[kind]).reshape(-1, 2)
    elif kind == "cf32" and a.dtype != np.complex64:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 2).view(np.complex64).reshape(-1)
    else:
        a = np.ascontiguousarray(a, _NP[kind])
    return a


def _alloc_like(x, kind: str, n: int):
    if _is_device(x):
        import torch
        dt = {"cf32": torch.complex64, "ci16": torch.int16, "ci32": torch.int32, "f32": torch.float32,
              "i16": torch.int16, "i32": torch.int32}[kind]
        shape = (n, 2) if kind in ("ci16", "ci32") else (n,)
        return torch.empty(shape, dtype=dt, device=x.device)
    if kind in ("ci16", "ci32"):
        return np.zeros((n, 2), _NP[kind])
    return np.zeros(n, _NP[kind])


def _ptr(x) -> C.c_void_p:
    if _is_device(x):
        if not x.is_contiguous():
            raise ValueError("device buffers must be contiguous")
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)


def _stream(x):
    import torch
    return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def _handles(objs):
    """The C array of the objects' handles, as the *_batched calls take it."""
    return (C.c_void_p * len(objs))(*[o._h.value for o in objs])


def _coeffs(c, kind: str) -> np.ndarray:
    return np.ascontiguousarray(c, _NP[kind])


class _Handle:
    _destroy = ""
    _clone = ""  # the C ABI's copy of the object with its state (the reference classes are value types)

    def __copy__(self):
        """A copy as the reference's implicit copy constructor makes it: the
        configuration AND the current streaming state (history, phase,
        registers), so the copy continues the stream like the original."""
        if not self._clone:
            raise TypeError(f"{type(self).__name__} is not copyable")
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__)
        c._h = C.c_void_p()
        A.call(self._clone, self._h, C.byref(c._h))
        return c

    def __deepcopy__(self, memo):
        return self.__copy__()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                getattr(A.lib(), self._destroy)(h)
            except Exception:
                pass
            self._h = C.c_void_p()


# ===================================================================== decimator
_DECIM_VARIANTS = {("cf32", "cf32", "cf32", "f32"): 0, ("ci16", "ci16", "ci32", "i32"): 1,
                   ("ci16", "ci16", "ci32", "i16"): 2, ("ci32", "ci16", "ci32", "i32"): 3}


class FilterDnsamplingFir(_Handle):
    """dsptl::FilterDnsamplingFir<InType, OutType, InternalType, CoefType, M>
    (dnsampling_filters.h:49-172).  ``abs_binding`` selects how coeffScaling
    sums |c| for float taps ('int' = canonical ::abs(int), 'fabs'); ``fp`` the
    float contract ('fma' = sequential FMA chain, 'strict' = mul then add)."""

    _destroy = "srcdsp_decim_destroy"
    _clone = "srcdsp_decim_clone"

    def __init__(self, coeffs, M: int = 4, InType="complex<float>", OutType="complex<float>",
                 InternalType="complex<float>", CoefType="float", abs_binding: str = "int", fp: str = "fma"):
        key = tuple(_kind(t) for t in (InType, OutType, InternalType, CoefType))
        if key not in _DECIM_VARIANTS:
            raise TypeError(f"FilterDnsamplingFir<{InType},{OutType},{InternalType},{CoefType}> "
                            "is not an instantiation the reference compiles (SURVEY §8c)")
        self.variant = _DECIM_VARIANTS[key]
        self.kin, self.kout, _, self.kc = key
        self.M = int(M)
        self.flags = (A.FLAG_ABS_FABS if abs_binding == "fabs" else 0) | (A.FLAG_FP_STRICT if fp == "strict" else 0)
        c = _coeffs(coeffs, self.kc)
        self._h = C.c_void_p()
        A.call("srcdsp_decim_create", C.byref(self._h), self.variant, self.M, c.ctypes.data, len(c), self.flags)
        self.ntaps = len(c)

    def setCoeffs(self, coeffs, require_multiple: bool = True):
        """dsptl_dnsampling_filters.h:114-134 (asserts N % M == 0)."""
        c = _coeffs(coeffs, self.kc)
        A.call("srcdsp_decim_set_coeffs", self._h, c.ctypes.data, len(c), int(require_multiple))
        self.ntaps = len(c)

    set_coeffs = setCoeffs

    def setLeftShiftBy2(self, left_shift: int):
        A.call("srcdsp_decim_set_left_shift", self._h, int(left_shift))

    set_left_shift = setLeftShiftBy2

    def reset(self):
        A.call("srcdsp_decim_reset", self._h)

    def state(self):
        cs, ls = C.c_uint(), C.c_int()
        hist = np.zeros(max(self.ntaps - 1, 0) * _BYTES[self.kin], np.uint8)
        A.call("srcdsp_decim_get_state", self._h, C.byref(cs), C.byref(ls),
               hist.ctypes.data if hist.size else None)
        return {"coeff_scaling": cs.value, "left_shift": ls.value, "history": hist}

    def step(self, inp, out=None):
        n_in = _nsamples(inp, self.kin)
        if out is None:
            out = _alloc_like(inp, self.kout, n_in // self.M)
        n_out = _nsamples(out, self.kout)
        if _is_device(inp):
            A.call("srcdsp_decim_step", self._h, _ptr(inp), n_in, _ptr(out), n_out, _stream(inp))
        else:
            x = _host(inp, self.kin)
            A.call("srcdsp_decim_step_host", self._h, _ptr(x), n_in, _ptr(out), n_out)
        return out


def decim_step_batched(filters, inp, out):
    """Step C same-configuration decimators over a [C, L] device batch in one
    launch (grid.y = channel)."""
    hs = _handles(filters)
    f0 = filters[0]
    ch = len(filters)
    n_in = _nsamples(inp, f0.kin) // ch
    n_out = _nsamples(out, f0.kout) // ch
    if n_out * f0.M != n_in:
        raise ValueError("batched decimator: output length * M must equal input length")
    A.call("srcdsp_decim_step_batched", hs, ch, _ptr(inp), n_in, _ptr(out), n_out, n_in, _stream(inp))
    return out


# ===================================================================== FilterFir
_FIR_VARIANTS = {("cf32", "cf32", "cf32", "f32"): 0, ("f32", "cf32", "f32", "f32"): 1,
                 ("ci16", "ci16", "ci32", "i32"): 2}


class FilterFir(_Handle):
    """::FilterFir<InType, OutType, InternalType, CoefType> (filters.h:42-169)."""

    _destroy = "srcdsp_fir_destroy"
    _clone = "srcdsp_fir_clone"

    def __init__(self, coeffs, InType="complex<float>", OutType="complex<float>", InternalType="complex<float>",
                 CoefType="float", abs_binding: str = "int", fp: str = "fma"):
        key = tuple(_kind(t) for t in (InType, OutType, InternalType, CoefType))
        if key not in _FIR_VARIANTS:
            raise TypeError(f"FilterFir<{InType},{OutType},{InternalType},{CoefType}> is not an instantiation "
                            "the reference compiles (filters.h:164 needs a complex output)")
        self.variant = _FIR_VARIANTS[key]
        self.kin, self.kout, _, self.kc = key
        flags = (A.FLAG_ABS_FABS if abs_binding == "fabs" else 0) | (A.FLAG_FP_STRICT if fp == "strict" else 0)
        c = _coeffs(coeffs, self.kc)
        self._h = C.c_void_p()
        A.call("srcdsp_fir_create", C.byref(self._h), self.variant, c.ctypes.data, len(c), flags)

    def setCoeffs(self, coeffs):
        c = _coeffs(coeffs, self.kc)
        A.call("srcdsp_fir_set_coeffs", self._h, c.ctypes.data, len(c))

    set_coeffs = setCoeffs

    def reset(self):
        A.call("srcdsp_fir_reset", self._h)

    def step(self, inp, out=None):
        n = _nsamples(inp, self.kin)
        if out is None:
            out = _alloc_like(inp, self.kout, n)
        n_out = _nsamples(out, self.kout)
        if _is_device(inp):
            A.call("srcdsp_fir_step", self._h, _ptr(inp), n, _ptr(out), n_out, _stream(inp))
        else:
            x = _host(inp, self.kin)
            A.call("srcdsp_fir_step_host", self._h, _ptr(x), n, _ptr(out), n_out)
        return out


# ============================================================ FilterUpsamplingFir
_UP_VARIANTS = {("ci16", "ci16", "ci32", "i32"): 0, ("ci16", "ci16", "ci32", "i16"): 1,
                ("i16", "i16", "i32", "i32"): 2}


class FilterUpsamplingFir(_Handle):
    """dsptl::FilterUpsamplingFir<InType, OutType, InternalType, CoefType, L>
    (upsampling_filters.h:36-326)."""

    _destroy = "srcdsp_up_destroy"
    _clone = "srcdsp_up_clone"

    def __init__(self, coeffs, L: int = 4, InType="complex<int16_t>", OutType="complex<int16_t>",
                 InternalType="complex<int32_t>", CoefType="int32_t"):
        key = tuple(_kind(t) for t in (InType, OutType, InternalType, CoefType))
        if key not in _UP_VARIANTS:
            raise TypeError(f"FilterUpsamplingFir<{InType},{OutType},{InternalType},{CoefType}> is not an "
                            "instantiation the reference compiles (dsp_complex.h:87 needs integer types)")
        self.variant = _UP_VARIANTS[key]
        self.kin, self.kout, _, self.kc = key
        self.L = int(L)
        c = _coeffs(coeffs, self.kc)
        self._h = C.c_void_p()
        A.call("srcdsp_up_create", C.byref(self._h), self.variant, self.L, c.ctypes.data, len(c))

    def setCoefficients(self, coeffs):
        c = _coeffs(coeffs, self.kc)
        A.call("srcdsp_up_set_coeffs", self._h, c.ctypes.data, len(c))

    def reset(self):
        A.call("srcdsp_up_reset", self._h)

    def _lengths(self):
        a, b, r = C.c_int(), C.c_int(), C.c_int()
        A.call("srcdsp_up_get_length", self._h, C.byref(a), C.byref(b), C.byref(r))
        return a.value, b.value, r.value

    def getLength(self):
        return self._lengths()[0]

    def getImpLength(self):
        return self._lengths()[1]

    def getUpsamplingRatio(self):
        return self._lengths()[2]

    length = property(getLength)

    def step(self, inp, out=None, flush: bool = False, iterator: bool = False):
        n = _nsamples(inp, self.kin)
        if out is None:
            extra = self.L * (self.getLength() // self.L) if flush else 0
            out = _alloc_like(inp, self.kout, n * self.L + extra)
        n_out = _nsamples(out, self.kout)
        if _is_device(inp):
            A.call("srcdsp_up_step", self._h, _ptr(inp), n, _ptr(out), n_out, int(flush), int(iterator),
                   _stream(inp))
        else:
            x = _host(inp, self.kin)
            A.call("srcdsp_up_step_host", self._h, _ptr(x), n, _ptr(out), n_out, int(flush), int(iterator))
        return out


# ========================================================================= Mixer
class Mixer(_Handle):
    """dsptl::Mixer<complex<int16_t>, complex<int16_t>, int16_t, N> (mixers.h:130-188)."""

    _destroy = "srcdsp_mixer_destroy"
    _clone = "srcdsp_mixer_clone"

    def __init__(self, N: int = 4096, InType="complex<int16_t>", OutType="complex<int16_t>", PhaseType="int16_t"):
        if (_kind(InType), _kind(OutType), _kind(PhaseType)) != ("ci16", "ci16", "i16"):
            raise TypeError("only Mixer<complex<int16_t>, complex<int16_t>, int16_t, N> is defined (mixers.h:120-131)")
        self.N = int(N)
        self._h = C.c_void_p()
        A.call("srcdsp_mixer_create", C.byref(self._h), self.N)

    def setFrequency(self, f):
        A.call("srcdsp_mixer_set_frequency", self._h, C.c_float(f))

    def reset(self, f=0.0):
        A.call("srcdsp_mixer_reset", self._h, C.c_float(f))

    def adjustFrequency(self, f=0.0):
        A.call("srcdsp_mixer_adjust_frequency", self._h, C.c_float(f))

    set_frequency, adjust_frequency = setFrequency, adjustFrequency

    def setPhase(self, phi: int):
        """Not a reference method: set the phase accumulator, e.g.
        to phaseAt(k) for a buffer segment starting at sample k."""
        A.call("srcdsp_mixer_set_phase", self._h, int(phi))

    def phaseAt(self, k: int) -> int:
        """Closed form of mixers.h:177: the phase after k samples from now."""
        phi, freq = self.state()[:2]
        return (phi + (k % self.N) * freq) % self.N

    def state(self):
        p, fr, nom = C.c_int(), C.c_int(), C.c_float()
        A.call("srcdsp_mixer_get_state", self._h, C.byref(p), C.byref(fr), C.byref(nom))
        return p.value, fr.value, nom.value

    def table(self):
        t = np.zeros(self.N, np.int16)
        A.call("srcdsp_mixer_get_table", self._h, t.ctypes.data_as(A.I16P))
        return t

    def step(self, inp, out=None):
        n = _nsamples(inp, "ci16")
        if out is None:
            out = _alloc_like(inp, "ci16", n)
        if _is_device(inp):
            A.call("srcdsp_mixer_step", self._h, _ptr(inp), n, _ptr(out), _stream(inp))
        else:
            x = _host(inp, "ci16")
            A.call("srcdsp_mixer_step_host", self._h, _ptr(x), n, _ptr(out))
        return out


class MixerDecimatorChain:
    """mixer.step(in, tmp); decim.step(tmp, out) fused into one device pass
    (config 4).  Both operators' state advances exactly as the two calls."""

    def __init__(self, mixer: Mixer, decim: FilterDnsamplingFir):
        self.mixer, self.decim = mixer, decim

    def step(self, inp, out=None):
        n = _nsamples(inp, "ci16")
        if out is None:
            out = _alloc_like(inp, "ci16", n // self.decim.M)
        if not _is_device(inp):
            return self.decim.step(self.mixer.step(inp), out)
        A.call("srcdsp_mixdecim_step", self.mixer._h, self.decim._h, _ptr(inp), n, _ptr(out),
               _nsamples(out, "ci16"), _stream(inp))
        return out


def mixdecim_step_batched(mixers, decims, inp, out):
    """Step C mixer -> decimator chains in one call (a DDC bank): channel c is
    exactly ``MixerDecimatorChain(mixers[c], decims[c]).step``.  ``inp`` of
    shape (L,) samples is one input shared by every channel (read once); of
    shape (C, L) one row per channel.  ``out`` is (C, L // M).  Device tensors
    of complex<int16_t> samples (int16 [..., 2])."""
    ch = len(mixers)
    if ch < 1 or len(decims) != ch:
        raise ValueError("DDC bank: need one decimator per mixer, at least one channel")
    if not (_is_device(inp) and _is_device(out)):
        raise ValueError("DDC bank: device tensors only")
    if inp.dim() not in (2, 3) or inp.shape[-1] != 2 or out.dim() != 3 or out.shape[-1] != 2:
        raise ValueError("DDC bank: inp is int16 [L, 2] (shared) or [C, L, 2], out int16 [C, L // M, 2]")
    shared = inp.dim() == 2
    if not shared and inp.shape[0] != ch:
        raise ValueError("DDC bank: one input row per channel")
    n_in = inp.shape[-2]
    M = decims[0].M
    if out.shape[0] != ch or out.shape[1] * M != n_in:
        raise ValueError("DDC bank: out must be [C, L // M] with L a multiple of M")
    hm = _handles(mixers)
    hd = _handles(decims)
    A.call("srcdsp_mixdecim_step_batched", hm, hd, ch, _ptr(inp), 0 if shared else n_in, _ptr(out), out.shape[1],
           n_in, _stream(inp))
    return out


def mixdecim_batched_stats():
    """(bank_calls, loop_calls): batched calls served by the DDC bank kernel and
    by the per-channel loop, process-wide."""
    b, l = C.c_ulong(), C.c_ulong()
    A.call("srcdsp_mixdecim_batched_stats", C.byref(b), C.byref(l))
    return b.value, l.value


def stream_set_grid_cap(cap: int):
    """Test and measurement hook: every launch of a persistent streaming kernel
    (the decimators, FilterFir on float input, the DDC bank) uses at most ``cap``
    workgroups in x, so a short call gives every workgroup several tiles
    (0: the product grids).  Process-wide; results do not depend on it."""
    A.call("srcdsp_stream_set_grid_cap", int(cap))


def stream_get_grid_cap() -> int:
    """The cap as last set by stream_set_grid_cap (0: the product grids)."""
    return int(A.lib().srcdsp_stream_get_grid_cap())


def stream_grid_stats():
    """(launches, looping): launches of the persistent streaming kernels, and
    those with more tiles than workgroups, process-wide."""
    a, b = C.c_ulong(), C.c_ulong()
    A.call("srcdsp_stream_grid_stats", C.byref(a), C.byref(b))
    return a.value, b.value


class UpsamplerMixerChain:
    """up.step(in, tmp, flush); mixer.step(tmp, out) fused into one device pass
    (the transmit chain).  Both operators' state advances exactly as the two
    calls.  ``out`` holds exactly L*n samples (L*(n + length/L) with flush)."""

    def __init__(self, up: FilterUpsamplingFir, mixer: Mixer):
        self.up, self.mixer = up, mixer

    def step(self, inp, out=None, flush: bool = False, iterator: bool = False):
        if not _is_device(inp):
            return self.mixer.step(self.up.step(inp, None, flush, iterator), out)
        n = _nsamples(inp, "ci16")
        if out is None:
            extra = self.up.L * (self.up.getLength() // self.up.L) if flush else 0
            out = _alloc_like(inp, "ci16", n * self.up.L + extra)
        A.call("srcdsp_upmix_step", self.up._h, self.mixer._h, _ptr(inp), n, _ptr(out), _nsamples(out, "ci16"),
               int(flush), int(iterator), _stream(inp))
        return out


def upmix_step_batched(ups, mixers, inp, out, flush: bool = False):
    """Step C interpolator -> mixer chains in one call (a transmitter bank):
    channel c is exactly ``UpsamplerMixerChain(ups[c], mixers[c]).step``.
    ``inp`` of shape [n, 2] is one baseband input shared by every channel; of
    shape [C, n, 2] one row per channel.  ``out`` is [C, >= L*(n + length/L
    when flushing), 2]; columns past a row's samples are left untouched.
    Device tensors of complex<int16_t> samples (int16 [..., 2])."""
    ch = len(ups)
    if ch < 1 or len(mixers) != ch:
        raise ValueError("upmix bank: need one mixer per interpolator, at least one channel")
    if not (_is_device(inp) and _is_device(out)):
        raise ValueError("upmix bank: device tensors only")
    if inp.dim() not in (2, 3) or inp.shape[-1] != 2 or out.dim() != 3 or out.shape[-1] != 2:
        raise ValueError("upmix bank: inp is int16 [n, 2] (shared) or [C, n, 2], out int16 [C, L*(n + flush), 2]")
    shared = inp.dim() == 2
    if (not shared and inp.shape[0] != ch) or out.shape[0] != ch:
        raise ValueError("upmix bank: one input row (or one shared input) and one output row per channel")
    n_in = inp.shape[-2]
    hu = _handles(ups)
    hm = _handles(mixers)
    A.call("srcdsp_upmix_step_batched", hu, hm, ch, _ptr(inp), 0 if shared else n_in, _ptr(out), out.shape[1],
           n_in, int(flush), _stream(inp))
    return out


def upmix_stats():
    """(fused_calls, pair_calls, bank_calls, loop_calls): single chain calls
    served by the fused kernel and by the pair of operators, batched calls
    served by one launch and by the per-channel loop, process-wide."""
    v = [C.c_ulong() for _ in range(4)]
    A.call("srcdsp_upmix_stats", *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


class RationalResampler:
    """up.step(in, tmp, flush); decim.step(tmp, out) in one call: the L/M rate
    change.  Both operators' state advances exactly as the two calls; ``tmp``
    is never the caller's.  ``out`` holds exactly L*n/M samples (L*(n +
    length/L)/M with flush), which must be whole.  Device tensors only."""

    def __init__(self, up: FilterUpsamplingFir, decim: FilterDnsamplingFir):
        self.up, self.decim = up, decim

    def step(self, inp, out=None, flush: bool = False):
        if not _is_device(inp):
            raise ValueError("RationalResampler: device tensors only")
        n = _nsamples(inp, "ci16")
        if out is None:
            n_mid = self.up.L * (n + (self.up.getLength() // self.up.L if flush else 0))
            if n_mid % self.decim.M:
                raise ValueError("RationalResampler: L*(n + length/L when flushing) must be a multiple of M")
            out = _alloc_like(inp, "ci16", n_mid // self.decim.M)
        A.call("srcdsp_resample_step", self.up._h, self.decim._h, _ptr(inp), n, _ptr(out), _nsamples(out, "ci16"),
               int(flush), _stream(inp))
        return out


def resample_step_batched(ups, decims, inp, out, flush: bool = False):
    """Step C interpolator -> decimator chains in one call: channel c is exactly
    ``RationalResampler(ups[c], decims[c]).step``.  ``inp`` is [C, n, 2], one
    row per channel; ``out`` is [C, >= L*(n + length/L when flushing)/M, 2],
    columns past a row's samples are left untouched.  Device tensors of
    complex<int16_t> samples (int16 [..., 2]); rows may be views of wider
    tensors (the row stride is taken from the tensor)."""
    ch = len(ups)
    if ch < 1 or len(decims) != ch:
        raise ValueError("resampler bank: need one decimator per interpolator, at least one channel")
    if not (_is_device(inp) and _is_device(out)):
        raise ValueError("resampler bank: device tensors only")
    if inp.dim() != 3 or inp.shape[-1] != 2 or out.dim() != 3 or out.shape[-1] != 2:
        raise ValueError("resampler bank: inp is int16 [C, n, 2], out int16 [C, L*(n + flush)/M, 2]")
    if inp.shape[0] != ch or out.shape[0] != ch:
        raise ValueError("resampler bank: one input row and one output row per channel")
    for x in (inp, out):
        if x.stride(2) != 1 or x.stride(1) != 2 or x.stride(0) % 2:
            raise ValueError("resampler bank: rows of contiguous samples")
    A.call("srcdsp_resample_step_batched", _handles(ups), _handles(decims), ch, C.c_void_p(inp.data_ptr()),
           inp.stride(0) // 2, C.c_void_p(out.data_ptr()), out.stride(0) // 2, inp.shape[1], int(flush), _stream(inp))
    return out


def resample_stats():
    """(fused_calls, pair_calls, bank_calls, loop_calls): single resampler calls
    served by the fused kernel and by the pair of operators, batched calls
    served by one launch and by the per-channel loop, process-wide."""
    v = [C.c_ulong() for _ in range(4)]
    A.call("srcdsp_resample_stats", *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def resample_geometry():
    """(tile_inputs, max_decim_taps) of the fused resampler kernel."""
    a, b = C.c_int(), C.c_int()
    A.call("srcdsp_resample_geometry", C.byref(a), C.byref(b))
    return a.value, b.value


def resample_set_min_tiles(min_tiles: int):
    """Test and measurement hook: send every call the fused resampler kernel
    takes with at least ``min_tiles`` tiles to it (0: the measured routing)."""
    A.call("srcdsp_resample_set_min_tiles", int(min_tiles))


# ================================================================ symbol mappers
def _bits(x):
    """Bits as the reference takes them: one uint8_t each, a one when non-zero."""
    if _is_device(x):
        import torch
        if x.dtype != torch.uint8:
            raise TypeError("device bits must be a uint8 tensor")
        return x
    return np.ascontiguousarray(x, np.uint8).reshape(-1)


class _SymbolMapper(_Handle):
    _destroy = "srcdsp_mapper_destroy"
    _clone = "srcdsp_mapper_clone"
    _kind_id = 0

    def __init__(self, T="int16_t"):
        if _kind(T) != "i16":
            raise TypeError("only the int16_t symbol mappers are provided (amplitude 8192, modulators.h:34-39)")
        self._h = C.c_void_p()
        A.call("srcdsp_mapper_create", C.byref(self._h), self._kind_id)

    def reset(self):
        A.call("srcdsp_mapper_reset", self._h)

    def state(self) -> int:
        k, s = C.c_int(), C.c_int()
        A.call("srcdsp_mapper_get_state", self._h, C.byref(k), C.byref(s))
        return s.value

    def setState(self, state: int):
        """Not a reference method: set the state (0..3) so a bit stream can be
        split in time."""
        A.call("srcdsp_mapper_set_state", self._h, int(state))

    def n_out(self, n_bits: int) -> int:
        return n_bits // 2 if self._kind_id == 1 else n_bits

    def step(self, bits, out=None):
        b = _bits(bits)
        n = b.numel() if _is_device(b) else b.size
        if out is None:
            if self._kind_id == 1 and n % 2:
                raise A.SrcdspError("srcdsp_mapper_step", A.ERR_SIZE, "a QPSK step takes an even number of bits")
            out = _alloc_like(b, "ci16", self.n_out(n))
        if _is_device(b):
            A.call("srcdsp_mapper_step", self._h, _ptr(b), n, _ptr(out), _nsamples(out, "ci16"), _stream(b))
        else:
            A.call("srcdsp_mapper_step_host", self._h, _ptr(b), n, _ptr(out), _nsamples(out, "ci16"))
        return out


class SymbolMapperSdpsk(_SymbolMapper):
    """dsptl::SymbolMapperSdpsk<int16_t> (modulators.h:82-131): one symbol per bit."""
    _kind_id = 0


class SymbolMapperQpsk(_SymbolMapper):
    """dsptl::SymbolMapperQpsk<int16_t> (modulators.h:147-198): one symbol per bit pair."""
    _kind_id = 1


def _bank_bits(bits, ch, who):
    if not _is_device(bits) or _bits(bits).dim() not in (1, 2):
        raise ValueError(f"{who}: bits is a uint8 device tensor [n] (shared) or [C, n]")
    shared = bits.dim() == 1
    if not shared and bits.shape[0] != ch:
        raise ValueError(f"{who}: one row of bits per channel")
    return shared, bits.shape[-1]


def mapper_step_batched(mappers, bits, out):
    """Step C symbol mappers of one kind in one call: row c is exactly
    ``mappers[c].step``.  ``bits`` of shape [n] is shared by every row; of
    shape [C, n] one row each.  ``out`` is int16 [C, >= symbols, 2]; columns
    past a row's symbols are left untouched.  Device tensors."""
    ch = len(mappers)
    if ch < 1:
        raise ValueError("mapper bank: at least one channel")
    shared, n = _bank_bits(bits, ch, "mapper bank")
    if not _is_device(out) or out.dim() != 3 or out.shape[-1] != 2 or out.shape[0] != ch:
        raise ValueError("mapper bank: out is an int16 device tensor [C, symbols, 2]")
    A.call("srcdsp_mapper_step_batched", _handles(mappers), ch, _ptr(bits), 0 if shared else n, _ptr(out),
           out.shape[1], n, _stream(bits))
    return out


class ModulatorChain:
    """mapper.step(bits, sym); up.step(sym, tmp, flush); mixer.step(tmp, out) in
    one call (the transmit chain from bits).  All three operators' state
    advances exactly as the three calls."""

    def __init__(self, mapper: _SymbolMapper, up: FilterUpsamplingFir, mixer: Mixer):
        self.mapper, self.up, self.mixer = mapper, up, mixer

    def step(self, bits, out=None, flush: bool = False, iterator: bool = False):
        if not _is_device(bits):
            return self.mixer.step(self.up.step(self.mapper.step(bits), None, flush, iterator), out)
        b = _bits(bits)
        n = b.numel()
        if out is None:
            extra = self.up.L * (self.up.getLength() // self.up.L) if flush else 0
            out = _alloc_like(b, "ci16", self.mapper.n_out(n) * self.up.L + extra)
        A.call("srcdsp_modulate_step", self.mapper._h, self.up._h, self.mixer._h, _ptr(b), n, _ptr(out),
               _nsamples(out, "ci16"), int(flush), int(iterator), _stream(b))
        return out


def modulate_step_batched(mappers, ups, mixers, bits, out, flush: bool = False):
    """Step C mapper -> interpolator -> mixer chains in one call: row c is
    exactly ``ModulatorChain(mappers[c], ups[c], mixers[c]).step``.  ``bits``
    [n] is shared, [C, n] one row per channel; ``out`` is int16 [C, >=
    L*(symbols + length/L when flushing), 2].  Device tensors."""
    ch = len(mappers)
    if ch < 1 or len(ups) != ch or len(mixers) != ch:
        raise ValueError("modulator bank: one mapper, interpolator and mixer per channel, at least one channel")
    shared, n = _bank_bits(bits, ch, "modulator bank")
    if not _is_device(out) or out.dim() != 3 or out.shape[-1] != 2 or out.shape[0] != ch:
        raise ValueError("modulator bank: out is an int16 device tensor [C, samples, 2]")
    A.call("srcdsp_modulate_step_batched", _handles(mappers), _handles(ups), _handles(mixers), ch, _ptr(bits),
           0 if shared else n, _ptr(out), out.shape[1], n, int(flush), _stream(bits))
    return out


def modulate_stats():
    """(fused_calls, chain_calls, bank_calls, loop_calls): single modulator
    calls served by the fused kernel and by the mapper followed by the
    interpolator -> mixer call, batched calls served by one launch and by the
    per-channel loop, process-wide."""
    v = [C.c_ulong() for _ in range(4)]
    A.call("srcdsp_modulate_stats", *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


# =========================================================== OQPSK Q-rail stagger
class QStagger(_Handle):
    """The offset of offset-QPSK (no reference class): a delay line of D
    samples, 1..64, on the imaginary rail of complex<int16_t> samples, between
    the interpolator and the mixer.  ``out[i] = (re(in[i]), im(in[i - D]))``,
    the first D imaginary halves coming from the carry of the step before."""

    _destroy = "srcdsp_stagger_destroy"
    _clone = "srcdsp_stagger_clone"

    def __init__(self, D: int):
        self._h = C.c_void_p()
        A.call("srcdsp_stagger_create", C.byref(self._h), int(D))
        self.D = int(D)

    def reset(self):
        A.call("srcdsp_stagger_reset", self._h)

    def state(self) -> np.ndarray:
        """The carry: the imaginary halves of the next step's first D outputs."""
        d = C.c_uint()
        carry = np.zeros(self.D, np.int16)
        A.call("srcdsp_stagger_get_state", self._h, C.byref(d), carry.ctypes.data_as(A.I16P))
        return carry

    def step(self, inp, out=None):
        n = _nsamples(inp, "ci16")
        if out is None:
            out = _alloc_like(inp, "ci16", n)
        if _is_device(inp):
            A.call("srcdsp_stagger_step", self._h, _ptr(inp), n, _ptr(out), _stream(inp))
        else:
            x = _host(inp, "ci16")
            A.call("srcdsp_stagger_step_host", self._h, _ptr(x), n, _ptr(out))
        return out


def stagger_geometry():
    """(tile_samples, max_delay) of the stagger's kernel."""
    t, d = C.c_int(), C.c_uint()
    A.call("srcdsp_stagger_geometry", C.byref(t), C.byref(d))
    return t.value, d.value


def stagger_step_batched(staggers, inp, out):
    """Step C staggers of one D in one call: row c is exactly
    ``staggers[c].step``.  ``inp`` int16 [n, 2] is shared by every row, [C, n,
    2] one row each; ``out`` is int16 [C, >= n, 2], columns past n untouched.
    Device tensors."""
    ch = len(staggers)
    if ch < 1:
        raise ValueError("stagger bank: at least one channel")
    if not (_is_device(inp) and _is_device(out)):
        raise ValueError("stagger bank: device tensors only")
    if inp.dim() not in (2, 3) or inp.shape[-1] != 2 or out.dim() != 3 or out.shape[-1] != 2:
        raise ValueError("stagger bank: inp is int16 [n, 2] (shared) or [C, n, 2], out int16 [C, n, 2]")
    shared = inp.dim() == 2
    if (not shared and inp.shape[0] != ch) or out.shape[0] != ch:
        raise ValueError("stagger bank: one input row (or one shared input) and one output row per channel")
    n = inp.shape[-2]
    A.call("srcdsp_stagger_step_batched", _handles(staggers), ch, _ptr(inp), 0 if shared else n, _ptr(out),
           out.shape[1], n, _stream(inp))
    return out


class OffsetModulatorChain:
    """mapper.step(bits, sym); up.step(sym, tmp, flush); stagger.step(tmp, tmp2);
    mixer.step(tmp2, out) in one call (the offset-QPSK transmit chain from
    bits).  All four operators' state advances exactly as the four calls."""

    def __init__(self, mapper: _SymbolMapper, up: FilterUpsamplingFir, stagger: QStagger, mixer: Mixer):
        self.mapper, self.up, self.stagger, self.mixer = mapper, up, stagger, mixer

    def step(self, bits, out=None, flush: bool = False, iterator: bool = False):
        if not _is_device(bits):
            y = self.up.step(self.mapper.step(bits), None, flush, iterator)
            return self.mixer.step(self.stagger.step(y), out)
        b = _bits(bits)
        n = b.numel()
        if out is None:
            extra = self.up.L * (self.up.getLength() // self.up.L) if flush else 0
            out = _alloc_like(b, "ci16", self.mapper.n_out(n) * self.up.L + extra)
        A.call("srcdsp_modulate_offset_step", self.mapper._h, self.up._h, self.stagger._h, self.mixer._h, _ptr(b), n,
               _ptr(out), _nsamples(out, "ci16"), int(flush), int(iterator), _stream(b))
        return out


def modulate_offset_step(mapper, up, stagger, mixer, bits, out=None, flush: bool = False, iterator: bool = False):
    """``OffsetModulatorChain(mapper, up, stagger, mixer).step(bits, out, flush, iterator)``."""
    return OffsetModulatorChain(mapper, up, stagger, mixer).step(bits, out, flush, iterator)


def modulate_offset_step_batched(mappers, ups, staggers, mixers, bits, out, flush: bool = False):
    """Step C mapper -> interpolator -> stagger -> mixer chains in one call:
    row c is exactly ``OffsetModulatorChain(mappers[c], ups[c], staggers[c],
    mixers[c]).step``.  ``bits`` [n] is shared, [C, n] one row per channel;
    ``out`` is int16 [C, >= L*(symbols + length/L when flushing), 2].  Device
    tensors."""
    ch = len(mappers)
    if ch < 1 or len(ups) != ch or len(staggers) != ch or len(mixers) != ch:
        raise ValueError("offset modulator bank: one mapper, interpolator, stagger and mixer per channel, at least "
                         "one channel")
    shared, n = _bank_bits(bits, ch, "offset modulator bank")
    if not _is_device(out) or out.dim() != 3 or out.shape[-1] != 2 or out.shape[0] != ch:
        raise ValueError("offset modulator bank: out is an int16 device tensor [C, samples, 2]")
    A.call("srcdsp_modulate_offset_step_batched", _handles(mappers), _handles(ups), _handles(staggers),
           _handles(mixers), ch, _ptr(bits), 0 if shared else n, _ptr(out), out.shape[1], n, int(flush),
           _stream(bits))
    return out


def modulate_offset_stats():
    """(fused_calls, chain_calls, bank_calls, loop_calls): single offset
    modulator calls served by the fused kernel and by the four operators,
    batched calls served by one launch and by the per-channel loop,
    process-wide."""
    v = [C.c_ulong() for _ in range(4)]
    A.call("srcdsp_modulate_offset_stats", *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


# ============================================================ carrier combiner
def combine(rows, out=None, shift: int = 0):
    """C carriers onto one wire (no reference call): ``out[i] =
    limitScale(sum_c rows[c][i], shift)``, the exact int32 sum shifted right
    arithmetically and clamped to int16, per component (dsp_complex.h:83-108).

    ``rows``: an int16 device tensor [C, n, 2] (its rows may be a view ``[:, :n]``
    of a wider buffer) or [n, 2] (one row), a list of [n, 2] device rows of one
    buffer at one spacing, or the same as host arrays.  ``out``: int16 [n, 2];
    it may be row 0 itself, and overlaps no other row.  Behind
    ``modulate_offset_step_batched`` it puts the bank's carriers onto the one
    row that ``mixdecim_step_batched`` takes as its shared input."""
    shift = int(shift)
    if isinstance(rows, (list, tuple)):
        if not rows:
            raise ValueError("combine: at least one row")
        if _is_device(rows[0]):
            n = _nsamples(rows[0], "ci16")
            if any(not _is_device(r) or not r.is_contiguous() or str(r.dtype) != "torch.int16" or
                   _nsamples(r, "ci16") != n for r in rows):
                raise ValueError("combine: the rows are contiguous int16 device tensors [n, 2] of one size")
            p = [r.data_ptr() for r in rows]
            step = p[1] - p[0] if len(p) > 1 else 0
            if step < 0 or step % 4 or any(b - a != step for a, b in zip(p, p[1:])):
                raise ValueError("combine: the rows lie in one buffer, one whole number of samples apart")
            first, ch, stride = rows[0], len(rows), step // 4
        else:
            rows = np.stack([_host(r, "ci16") for r in rows])
    if not isinstance(rows, (list, tuple)):
        if _is_device(rows):
            t = rows if rows.dim() == 3 else rows.unsqueeze(0)
            if t.dim() != 3 or t.shape[-1] != 2 or str(t.dtype) != "torch.int16" or t.shape[0] < 1:
                raise ValueError("combine: rows is an int16 tensor [C, n, 2] or [n, 2]")
            ch, n = t.shape[0], t.shape[1]
            st = t.stride()
            if n and (st[2] != 1 or (n > 1 and st[1] != 2) or (ch > 1 and (st[0] % 2 or st[0] < 0))):
                raise ValueError("combine: samples are contiguous within a row, rows a whole number of samples apart")
            first, stride = t[0], (st[0] // 2 if ch > 1 else 0)
        else:
            a = np.ascontiguousarray(rows, np.int16)
            a = a.reshape((1,) + a.shape) if a.ndim == 2 else a
            if a.ndim != 3 or a.shape[-1] != 2 or a.shape[0] < 1:
                raise ValueError("combine: rows is int16 [C, n, 2] or [n, 2]")
            if out is None:
                out = np.zeros(a.shape[1:], np.int16)
            if _is_device(out) or out.dtype != np.int16 or not out.flags.c_contiguous or out.size != 2 * a.shape[1]:
                raise ValueError("combine: out is a contiguous int16 host array [n, 2]")
            A.call("srcdsp_combine_step_host", _ptr(a), a.shape[1], a.shape[0], _ptr(out), a.shape[1], shift)
            return out
    if out is None:
        out = _alloc_like(first, "ci16", n)
    if not _is_device(out) or str(out.dtype) != "torch.int16" or not out.is_contiguous() or \
            _nsamples(out, "ci16") != n:
        raise ValueError("combine: out is a contiguous int16 device tensor [n, 2]")
    A.call("srcdsp_combine_step", C.c_void_p(first.data_ptr()), stride, ch, _ptr(out), n, shift, _stream(out))
    return out


# ===================================================== summing modulator bank
def modulate_sum_step(mappers, ups, staggers, mixers, bits, out=None, shift: int = 0, flush: bool = False):
    """C transmit chains from bits onto one wire in one call: ``out`` is what
    ``modulate_offset_step_batched`` into C rows (``staggers=None``:
    ``modulate_step_batched``) and ``combine(rows, out, shift)`` leave, and every
    handle ends as the bank leaves it, without the [C, n_out] rows.  ``bits``
    [n] is shared, [C, n] one row per channel (its rows may be a view ``[:, :n]``
    of a wider buffer); ``out`` is int16 [L*(symbols + length/L when flushing),
    2], made when None.  Device tensors."""
    ch = len(mappers)
    if ch < 1 or len(ups) != ch or len(mixers) != ch or (staggers is not None and len(staggers) != ch):
        raise ValueError("summing modulator bank: one mapper, interpolator, stagger (or None for all) and mixer per "
                         "channel, at least one channel")
    shared, n = _bank_bits(bits, ch, "summing modulator bank")
    stride = 0
    if not shared:
        if (n and bits.stride(1) != 1) or (ch > 1 and bits.stride(0) < n):
            raise ValueError("summing modulator bank: bits are contiguous within a row, rows at least n apart")
        stride = bits.stride(0) if ch > 1 else n
    if out is None:
        up = ups[0]
        extra = up.L * (up.getLength() // up.L) if flush else 0
        out = _alloc_like(bits, "ci16", mappers[0].n_out(n) * up.L + extra)
    if not _is_device(out) or str(out.dtype) != "torch.int16" or not out.is_contiguous():
        raise ValueError("summing modulator bank: out is a contiguous int16 device tensor [n_out, 2]")
    A.call("srcdsp_modulate_sum_step", _handles(mappers), _handles(ups),
           _handles(staggers) if staggers is not None else None, _handles(mixers), ch, C.c_void_p(bits.data_ptr()),
           stride, _ptr(out), _nsamples(out, "ci16"), n, int(flush), int(shift), _stream(bits))
    return out


def modulate_sum_stats():
    """(fused_calls, bank_calls): summing modulator calls served by the fused
    kernel and by the bank followed by the combiner, process-wide."""
    v = [C.c_ulong() for _ in range(2)]
    A.call("srcdsp_modulate_sum_stats", *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def modulate_sum_geometry(L: int):
    """(tile_symbols, min_tiles, max_channels): the symbols one workgroup of the
    fused kernel covers, and the calls it serves of those it takes at
    interpolation by L: at least min_tiles tiles (0: none), at most
    max_channels chains."""
    t, a, b = C.c_int(), C.c_long(), C.c_int()
    A.call("srcdsp_modulate_sum_geometry", int(L), C.byref(t), C.byref(a), C.byref(b))
    return t.value, a.value, b.value


def modulate_sum_set_min_tiles(min_tiles: int):
    """Route every call the fused kernel takes to it from ``min_tiles`` tiles
    on, process-wide (tests, measurements); 0 puts the measured routing back.
    Results do not depend on the routing."""
    A.call("srcdsp_modulate_sum_set_min_tiles", int(min_tiles))


# ======================================================== FixedPatternCorrelator
class FixedPatternCorrelator(_Handle):
    """dsptl::FixedPatternCorrelator<int16_t, int32_t, N, S> (correlators.h:54-316)."""

    _destroy = "srcdsp_corr_destroy"
    _clone = "srcdsp_corr_clone"

    def __init__(self, N: int = 32, S: int = 4, InType="int16_t", CompType="int32_t"):
        if (_kind(InType), _kind(CompType)) != ("i16", "i32"):
            raise TypeError("FixedPatternCorrelator is provided for <int16_t, int32_t, N, S>")
        self.N, self.S = int(N), int(S)
        self._h = C.c_void_p()
        A.call("srcdsp_corr_create", C.byref(self._h), self.N, self.S)

    def setPattern(self, pattern, thresholdCoeff: float = 0.8):
        p = np.ascontiguousarray(pattern, np.int32).reshape(-1, 2)
        if len(p) != self.N:
            raise ValueError(f"pattern must have N={self.N} complex<int32_t> entries")
        A.call("srcdsp_corr_set_pattern", self._h, p.ctypes.data_as(A.I32P), C.c_double(thresholdCoeff))

    set_pattern = setPattern

    def reset(self):
        A.call("srcdsp_corr_reset", self._h)

    def step(self, inp):
        """Returns (found, corrIndex); corrIndex is meaningful only if found."""
        n = _nsamples(inp, "ci16")
        found, idx = C.c_int(0), C.c_int(-1)
        if _is_device(inp):
            A.call("srcdsp_corr_step", self._h, _ptr(inp), n, C.byref(found), C.byref(idx), _stream(inp))
        else:
            x = _host(inp, "ci16")
            A.call("srcdsp_corr_step_host", self._h, _ptr(x), n, C.byref(found), C.byref(idx))
        return bool(found.value), idx.value

    def stepAll(self, inp, max_hits: int):
        """Not a reference method: every detection the loop of step() on the
        remainders makes in `inp`, at most `max_hits` of them, in one call.
        Returns (indices, bits, consumed): the corrIndex of each detection
        relative to `inp` (int array [k]), the bitSamples of each (int16
        [k, N, 2]) and the samples the loop processed (< len(inp) only when
        max_hits was reached; stepAll(inp[consumed:]) continues)."""
        n, mh = _nsamples(inp, "ci16"), int(max_hits)
        mh = min(mh, n // 2 + 1)  # detections lie at least two samples apart: no more rows are ever filled
        k, used = C.c_int(0), C.c_size_t(0)
        idx = np.zeros(max(mh, 1), np.intc)
        bits = np.zeros((max(mh, 1), self.N, 2), np.int16)
        ip, bp = idx.ctypes.data_as(A.IP), bits.ctypes.data_as(A.I16P)
        if _is_device(inp):
            A.call("srcdsp_corr_step_all", self._h, _ptr(inp), n, mh, C.byref(k), ip, bp, C.byref(used),
                   _stream(inp))
        else:
            x = _host(inp, "ci16")
            A.call("srcdsp_corr_step_all_host", self._h, _ptr(x), n, mh, C.byref(k), ip, bp, C.byref(used))
        return idx[:k.value].copy(), bits[:k.value].copy(), used.value

    step_all = stepAll

    def step_trace(self, inp):
        """step() as the reference's CREATE_DEBUG_FILES build runs it
        (correlators.h:253-257): (found, corrIndex, corr, energy), where corr[k]
        / energy[k] are corrValue[0] / energyValue[0] after each processed
        input sample (numpy uint32)."""
        n = _nsamples(inp, "ci16")
        found, idx, cnt = C.c_int(0), C.c_int(-1), C.c_size_t(0)
        corr, en = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        cp, ep = corr.ctypes.data_as(A.U32P), en.ctypes.data_as(A.U32P)
        if _is_device(inp):
            A.call("srcdsp_corr_step_trace", self._h, _ptr(inp), n, C.byref(found), C.byref(idx), cp, ep,
                   C.byref(cnt), _stream(inp))
        else:
            x = _host(inp, "ci16")
            A.call("srcdsp_corr_step_host_trace", self._h, _ptr(x), n, C.byref(found), C.byref(idx), cp, ep,
                   C.byref(cnt))
        k = cnt.value
        return bool(found.value), idx.value, corr[:k], en[:k]

    def prime(self, inp):
        """Not a reference method: leave the state step() would
        leave after streaming `inp` with no detection test -- seeds a time
        segment of a split buffer with its halo.  Device input only."""
        if not _is_device(inp):
            raise TypeError("prime() takes a device-resident buffer")
        A.call("srcdsp_corr_prime", self._h, _ptr(inp), _nsamples(inp, "ci16"), _stream(inp))

    def getRefBitSamples(self):
        b = np.zeros((self.N, 2), np.int16)
        A.call("srcdsp_corr_get_bit_samples", self._h, b.ctypes.data_as(A.I16P))
        return b

    bit_samples = getRefBitSamples

    def getStatus(self):
        e3, c3 = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
        ce, cs, tf = C.c_uint32(), C.c_int(), C.c_double()
        A.call("srcdsp_corr_get_status", self._h, e3, c3, C.byref(ce), C.byref(cs), C.byref(tf))
        return {"energy": list(e3), "corr": list(c3), "coeffs_energy": ce.value, "coeff_scaling": cs.value,
                "threshold_factor": tf.value}

    status = getStatus


def corr_step_batched(correlators, inp):
    """Step C correlators in one call: channel c is exactly
    ``correlators[c].step(inp_c)``, each scanning up to its own first
    detection.  ``inp`` is a device tensor of complex<int16_t> samples: int16
    [n, 2], one input every channel scans (several patterns searched in one
    stream), or [C, n, 2], one contiguous row per channel.  The correlators
    share N and S; patterns may differ.  Returns a list of (found, corrIndex),
    corrIndex meaningful only if found."""
    ch = len(correlators)
    if ch < 1:
        raise ValueError("corr_step_batched: at least one correlator")
    if not _is_device(inp):
        raise TypeError("corr_step_batched() takes a device-resident buffer")
    if inp.dim() not in (2, 3) or inp.shape[-1] != 2 or inp.element_size() != 2:
        raise ValueError("corr_step_batched: inp is int16 [n, 2] (shared) or [C, n, 2]")
    shared = inp.dim() == 2
    if not shared and inp.shape[0] != ch:
        raise ValueError("corr_step_batched: one input row per correlator")
    n = inp.shape[-2]
    hs = _handles(correlators)
    found, idx = (C.c_int * ch)(), (C.c_int * ch)(*([-1] * ch))
    A.call("srcdsp_corr_step_batched", hs, ch, _ptr(inp), 0 if shared else n, n, found, idx, _stream(inp))
    return [(bool(found[c]), idx[c]) for c in range(ch)]


def corr_step_all_batched(correlators, inp, max_hits: int):
    """FixedPatternCorrelator.stepAll for C correlators in one call: channel c
    is exactly ``correlators[c].stepAll(inp_c, max_hits)``.  ``inp`` as for
    corr_step_batched: int16 [n, 2] (one shared input) or [C, n, 2], on the
    device.  Returns a list of (indices, bits, consumed) per channel."""
    ch, mh = len(correlators), int(max_hits)
    if ch < 1:
        raise ValueError("corr_step_all_batched: at least one correlator")
    if not _is_device(inp):
        raise TypeError("corr_step_all_batched() takes a device-resident buffer")
    if inp.dim() not in (2, 3) or inp.shape[-1] != 2 or inp.element_size() != 2:
        raise ValueError("corr_step_all_batched: inp is int16 [n, 2] (shared) or [C, n, 2]")
    shared = inp.dim() == 2
    if not shared and inp.shape[0] != ch:
        raise ValueError("corr_step_all_batched: one input row per correlator")
    n, N = inp.shape[-2], correlators[0].N
    mh = min(mh, n // 2 + 1)  # detections lie at least two samples apart: no more rows are ever filled
    hs = _handles(correlators)
    k, used = (C.c_int * ch)(), (C.c_size_t * ch)()
    idx = np.zeros((ch, max(mh, 1)), np.intc)
    bits = np.zeros((ch, max(mh, 1), N, 2), np.int16)
    A.call("srcdsp_corr_step_all_batched", hs, ch, _ptr(inp), 0 if shared else n, n, mh, k,
           idx.ctypes.data_as(A.IP), bits.ctypes.data_as(A.I16P), used, _stream(inp))
    return [(idx[c, :k[c]].copy(), bits[c, :k[c]].copy(), used[c]) for c in range(ch)]


def corr_all_stats():
    """(kernel_calls, loop_calls): stepAll calls served by the candidate and
    resolve kernels and by the loop of srcdsp_corr_step, process-wide."""
    b, l = C.c_ulong(), C.c_ulong()
    A.call("srcdsp_corr_all_stats", C.byref(b), C.byref(l))
    return b.value, l.value


def corr_batched_stats():
    """(bank_calls, loop_calls): batched correlator calls served by the bank
    kernel and by the per-channel loop, process-wide."""
    b, l = C.c_ulong(), C.c_ulong()
    A.call("srcdsp_corr_batched_stats", C.byref(b), C.byref(l))
    return b.value, l.value


# ============================================================== DemodulatorOqpsk
class DemodulatorOqpsk(_Handle):
    """dsptl::DemodulatorOqpsk<int16_t> (demodulators.h:53-130): one sample per
    bit in, soft bits (int8) out.  One burst is a sequential recurrence and
    runs on one GPU lane: a single step() is slower than a host core.  Step
    many bursts at once with demod_step_batched()."""

    _destroy = "srcdsp_demod_destroy"
    _clone = "srcdsp_demod_clone"

    def __init__(self, InType="int16_t"):
        if _kind(InType) != "i16":
            raise TypeError("DemodulatorOqpsk is provided for <int16_t>")
        self._h = C.c_void_p()
        A.call("srcdsp_demod_create", C.byref(self._h))

    def setSyncPattern(self, bits):
        b = np.ascontiguousarray(bits, np.int8).reshape(-1)
        A.call("srcdsp_demod_set_sync_pattern", self._h, b.ctypes.data_as(C.POINTER(C.c_int8)), len(b))

    def setReference(self, ref):
        """ref: complex<int16_t> samples, int16 [n, 2] -- or a
        FixedPatternCorrelator, whose bit samples (getRefBitSamples) are taken
        from its handle."""
        if isinstance(ref, FixedPatternCorrelator):
            A.call("srcdsp_demod_set_reference_corr", self._h, ref._h, None)
            return
        r = np.ascontiguousarray(ref, np.int16).reshape(-1, 2)
        A.call("srcdsp_demod_set_reference", self._h, r.ctypes.data_as(A.I16P), len(r))

    def setInitialFrequency(self, f: float):
        A.call("srcdsp_demod_set_initial_frequency", self._h, C.c_float(f))

    def setInitialPhase(self, p: float):
        A.call("srcdsp_demod_set_initial_phase", self._h, C.c_float(p))

    def setInputShift(self, shift: int):
        A.call("srcdsp_demod_set_input_shift", self._h, int(shift))

    def reset(self):
        A.call("srcdsp_demod_reset", self._h)

    def getMeasuredFrequency(self) -> float:
        f = C.c_float()
        A.call("srcdsp_demod_get_measured_frequency", self._h, C.byref(f))
        return f.value

    set_sync_pattern, set_reference, set_initial_frequency = setSyncPattern, setReference, setInitialFrequency
    set_initial_phase, set_input_shift, measured_frequency = setInitialPhase, setInputShift, getMeasuredFrequency

    def state(self):
        """(bitCnt, mod2Cnt, phase, bit1, bit2, Iprev, Qprev, intialFreqEst,
        accumulatedFrequency, rightShift)."""
        bc = C.c_uint()
        v = [C.c_int() for _ in range(9)]
        A.call("srcdsp_demod_get_state", self._h, C.byref(bc), *[C.byref(x) for x in v])
        return (bc.value,) + tuple(x.value for x in v)

    def step(self, inp):
        """Returns (soft bits, error): an int8 device tensor for a device
        input, an int8 numpy array for a host one."""
        n = _nsamples(inp, "ci16")
        ns, err = C.c_size_t(0), C.c_int32(0)
        if _is_device(inp):
            import torch
            soft = torch.empty(max(n, 1), dtype=torch.int8, device=inp.device)
            A.call("srcdsp_demod_step", self._h, _ptr(inp), n, _ptr(soft), n, C.byref(ns), C.byref(err), _stream(inp))
        else:
            x = _host(inp, "ci16")
            soft = np.zeros(max(n, 1), np.int8)
            A.call("srcdsp_demod_step_host", self._h, _ptr(x), n, _ptr(soft), n, C.byref(ns), C.byref(err))
        return soft[:ns.value], err.value


def demod_tables():
    """(sineLUT int16[8192], phaseLUT int16[128 * 128]) as the library built them."""
    s, p = np.zeros(8192, np.int16), np.zeros(128 * 128, np.int16)
    A.call("srcdsp_demod_get_tables", s.ctypes.data_as(A.I16P), p.ctypes.data_as(A.I16P))
    return s, p


def demod_step_batched(demods, x, offsets=None, n=None):
    """Step C demodulators in one launch: channel c is exactly
    ``demods[c].step(x_c)``.  ``x`` is a device tensor of complex<int16_t>
    samples: int16 [C, m, 2], one row per channel, or [m, 2], one buffer every
    channel reads (frequency hypotheses of one burst).  ``offsets[c]`` (samples)
    moves channel c's first sample within its row; every channel steps ``n``
    samples (default: what the largest offset leaves of a row).  Returns
    (soft int8 [C, n] device tensor, n_soft list, errors list): row c holds
    n_soft[c] soft bits."""
    import torch
    ch = len(demods)
    if ch < 1:
        raise ValueError("demod_step_batched: at least one demodulator")
    if not _is_device(x):
        raise TypeError("demod_step_batched() takes a device-resident buffer")
    if x.dim() not in (2, 3) or x.shape[-1] != 2 or x.element_size() != 2:
        raise ValueError("demod_step_batched: x is int16 [m, 2] (shared) or [C, m, 2]")
    shared = x.dim() == 2
    if not shared and x.shape[0] != ch:
        raise ValueError("demod_step_batched: one input row per demodulator")
    m = x.shape[-2]
    offs = [0] * ch if offsets is None else [int(o) for o in offsets]
    if len(offs) != ch or min(offs) < 0 or max(offs) > m:
        raise ValueError("demod_step_batched: one offset per channel, within the row")
    if n is None:
        n = m - max(offs)
    if n < 0 or max(offs) + n > m:
        raise ValueError("demod_step_batched: offset + n runs past the row")
    hs = _handles(demods)
    off = (C.c_size_t * ch)(*offs)
    ns, err = (C.c_size_t * ch)(), (C.c_int32 * ch)()
    soft = torch.empty((ch, max(n, 1)), dtype=torch.int8, device=x.device)
    A.call("srcdsp_demod_step_batched", hs, ch, _ptr(x), 0 if shared else m, off, n, _ptr(soft), max(n, 1), ns, err,
           _stream(x))
    return soft[:, :n], list(ns), list(err)


# ============================================================== DemodulatorSdpsk
class DemodulatorSdpsk(_Handle):
    """The receiver of SymbolMapperSdpsk (no reference class): bit = sign of
    Im(x[i] * conj(x[i - D])), D samples per symbol (1..64); the soft bit is
    that product shifted right by ``shift`` (0..31) and clamped to int8.  No
    PLL: every output is independent.  The first D outputs after a reset read
    the zero carry and are 0."""

    _destroy = "srcdsp_sdpsk_destroy"
    _clone = "srcdsp_sdpsk_clone"

    def __init__(self, D: int = 1, shift: int = 0):
        self._h = C.c_void_p()
        A.call("srcdsp_sdpsk_create", C.byref(self._h), int(D), int(shift))
        self.D = int(D)

    def reset(self):
        A.call("srcdsp_sdpsk_reset", self._h)

    def setShift(self, shift: int):
        A.call("srcdsp_sdpsk_set_shift", self._h, int(shift))

    set_shift = setShift

    def state(self):
        """(D, shift, carry int16 [D, 2]): the carry is the last D samples seen."""
        d, s = C.c_uint(), C.c_uint()
        carry = np.zeros((self.D, 2), np.int16)
        A.call("srcdsp_sdpsk_get_state", self._h, C.byref(d), C.byref(s), carry.ctypes.data_as(A.I16P))
        return d.value, s.value, carry

    def step(self, inp):
        """Returns (soft int8 [n], bits uint8 [n]): device tensors for a device
        input (asynchronous on torch's current stream), numpy arrays for a host
        one."""
        n = _nsamples(inp, "ci16")
        if _is_device(inp):
            import torch
            soft = torch.empty(n, dtype=torch.int8, device=inp.device)
            bits = torch.empty(n, dtype=torch.uint8, device=inp.device)
            A.call("srcdsp_sdpsk_step", self._h, _ptr(inp), n, _ptr(soft), _ptr(bits), _stream(inp))
        else:
            x = _host(inp, "ci16")
            soft, bits = np.zeros(n, np.int8), np.zeros(n, np.uint8)
            A.call("srcdsp_sdpsk_step_host", self._h, _ptr(x), n, _ptr(soft), _ptr(bits))
        return soft, bits


def sdpsk_geometry():
    """(tile_samples, max_lag, workgroups) of the SDPSK demodulator's kernel;
    workgroups is 0: the kernel is not persistent."""
    t, d, w = C.c_int(), C.c_uint(), C.c_int()
    A.call("srcdsp_sdpsk_geometry", C.byref(t), C.byref(d), C.byref(w))
    return t.value, d.value, w.value


def sdpsk_step_batched(demods, x, offsets=None, n=None):
    """Step C SDPSK demodulators of one D and shift in one call: row c is
    exactly ``demods[c].step(x_c)``.  ``x`` is a device tensor of
    complex<int16_t> samples: int16 [C, m, 2], one row per channel, or [m, 2],
    one buffer every channel reads (all the hits of one stream).  ``offsets[c]``
    (samples) moves channel c's first sample within its row; every channel
    steps ``n`` samples (default: what the largest offset leaves of a row).
    Returns (soft int8 [C, n], bits uint8 [C, n]) device tensors."""
    import torch
    ch = len(demods)
    if ch < 1:
        raise ValueError("sdpsk_step_batched: at least one demodulator")
    if not _is_device(x):
        raise TypeError("sdpsk_step_batched() takes a device-resident buffer")
    if x.dim() not in (2, 3) or x.shape[-1] != 2 or x.element_size() != 2:
        raise ValueError("sdpsk_step_batched: x is int16 [m, 2] (shared) or [C, m, 2]")
    shared = x.dim() == 2
    if not shared and x.shape[0] != ch:
        raise ValueError("sdpsk_step_batched: one input row per demodulator")
    m = x.shape[-2]
    offs = [0] * ch if offsets is None else [int(o) for o in offsets]
    if len(offs) != ch or min(offs) < 0 or max(offs) > m:
        raise ValueError("sdpsk_step_batched: one offset per channel, within the row")
    if n is None:
        n = m - max(offs)
    if n < 0 or max(offs) + n > m:
        raise ValueError("sdpsk_step_batched: offset + n runs past the row")
    stride = (max(n, 1) + 3) & ~3  # rows on 4-byte boundaries: whole-word stores
    soft = torch.empty((ch, stride), dtype=torch.int8, device=x.device)
    bits = torch.empty((ch, stride), dtype=torch.uint8, device=x.device)
    A.call("srcdsp_sdpsk_step_batched", _handles(demods), ch, _ptr(x), 0 if shared else m, (C.c_size_t * ch)(*offs), n,
           _ptr(soft), stride, _ptr(bits), stride, _stream(x))
    return soft[:, :n], bits[:, :n]


# ================================================================== estimateFreq
class FreqEstimator(_Handle):
    """estimateFreq<int16_t, L> (dsptl_miscellaneous.h:43-58): the frequency of
    complex<int16_t> samples in rad/sample from their lag-L autocorrelation
    (-w for e^{+jwn}, as the reference).  The sums are exact 64-bit integers;
    ``exact`` tells that the float is the reference's bit for bit
    (include/srcdsp_hip.h).  The handle holds L and scratch, no signal state."""

    _destroy = "srcdsp_freqest_destroy"

    def __init__(self, L: int = 1, InType="int16_t"):
        if _kind(InType) != "i16":
            raise TypeError("estimateFreq is provided for <int16_t, L>")
        self.L = int(L)
        self._h = C.c_void_p()
        A.call("srcdsp_freqest_create", C.byref(self._h), self.L)

    def geometry(self, device: bool = True):
        """(tile, vec, workgroups): pairs per tile, samples per vector load and
        (device=True) the persistent workgroups of a launch on this device."""
        t, v, w = C.c_int(), C.c_int(), C.c_int()
        A.call("srcdsp_freqest_geometry", self._h, None, C.byref(t), C.byref(v), C.byref(w) if device else None)
        return t.value, v.value, w.value

    def run(self, x):
        """(freq, (sumI, sumQ), exact) of one buffer: a device tensor or a host
        array of complex<int16_t> samples, int16 [n, 2]."""
        n = _nsamples(x, "ci16")
        f, s, e = C.c_float(), (C.c_int64 * 2)(), C.c_int()
        if _is_device(x):
            A.call("srcdsp_freqest_run", self._h, _ptr(x), n, C.byref(f), s, C.byref(e), _stream(x))
        else:
            h = _host(x, "ci16")
            A.call("srcdsp_freqest_run_host", self._h, _ptr(h), n, C.byref(f), s, C.byref(e))
        return np.float32(f.value), (s[0], s[1]), bool(e.value)

    def run_batched(self, x, offsets=None, n=None, shared=False):
        """C rows in one launch.  ``x`` is a device tensor of complex<int16_t>
        samples: int16 [C, m, 2], one row per channel, or with ``shared`` [m, 2],
        one buffer every row lies in (one row per offset).  ``offsets[c]``
        (samples) moves row c's first sample; every row has ``n`` samples
        (default: what the largest offset leaves).  Returns (freq float32 [C],
        sums int64 [C, 2], exact bool [C]), row c as ``run`` of that row."""
        if not _is_device(x):
            raise TypeError("FreqEstimator.run_batched() takes a device-resident buffer")
        if x.dim() != (2 if shared else 3) or x.shape[-1] != 2 or x.element_size() != 2:
            raise ValueError("FreqEstimator.run_batched: x is int16 [C, m, 2], or [m, 2] with shared")
        m = x.shape[-2]
        if shared:
            if offsets is None:
                raise ValueError("FreqEstimator.run_batched: a shared buffer needs one offset per row")
            ch = len(offsets)
        else:
            ch = x.shape[0]
        if ch < 1:
            raise ValueError("FreqEstimator.run_batched: at least one row")
        offs = [0] * ch if offsets is None else [int(o) for o in offsets]
        if len(offs) != ch or min(offs) < 0 or max(offs) > m:
            raise ValueError("FreqEstimator.run_batched: one offset per row, within the row")
        if n is None:
            n = m - max(offs)
        if n < 0 or max(offs) + n > m:
            raise ValueError("FreqEstimator.run_batched: offset + n runs past the row")
        f, s, e = np.zeros(ch, np.float32), np.zeros((ch, 2), np.int64), np.zeros(ch, np.intc)
        off = None if offsets is None else (C.c_size_t * ch)(*offs)
        A.call("srcdsp_freqest_run_batched", self._h, ch, _ptr(x), 0 if shared else m, off, n,
               f.ctypes.data_as(A.FP), s.ctypes.data_as(C.POINTER(C.c_int64)), e.ctypes.data_as(A.IP), _stream(x))
        return f, s, e.astype(bool)


def estimate_freq(x, L: int = 1):
    """estimateFreq<int16_t, L>(x) (dsptl_miscellaneous.h:43-58) as float32."""
    return FreqEstimator(L).run(x)[0]


def demod_acquire_batched(demods, cors, found=None, L=1, first=1, scale=-1.0):
    """The join of corr_step_batched and demod_step_batched.  For every channel
    c taken (``found`` None, or found[c] true): demods[c] takes cors[c]'s bit
    samples as its reference, estimateFreq<int16_t, L> over bit samples
    first .. N-1 times ``scale`` as its initial frequency, and is reset.
    ``first=1`` leaves out slot 0 of the bit samples, which is the detected
    sample and not a preamble sample; ``scale=-1`` turns the estimator's sign
    (-w for e^{+jwn}) into the demodulator's.  All or nothing (SrcdspError and
    no handle changed).  Returns the estimates, float32 [C] (nan where not
    taken).  Host code: no launch."""
    ch = len(demods)
    if ch < 1 or len(cors) != ch:
        raise ValueError("demod_acquire_batched: one correlator per demodulator, at least one")
    if found is not None and len(found) != ch:
        raise ValueError("demod_acquire_batched: one found flag per channel")
    hd = _handles(demods)
    hc = _handles(cors)
    fl = None if found is None else (C.c_int * ch)(*[int(bool(v)) for v in found])
    f = np.full(ch, np.nan, np.float32)
    A.call("srcdsp_demod_acquire_batched", hd, hc, ch, fl, int(L), int(first), C.c_float(scale),
           f.ctypes.data_as(A.FP))
    return f


def fill_synthetic(t, kind: str, seed: int = 0x5EED, channel: int = 0, offset: int = 0, lo: int = -2048,
                   hi: int = 2047):
    """Fill a device tensor with the counter-based synthetic samples."""
    k = {"cf32": 0, "ci16": 1}[kind]
    n = _nsamples(t, kind)
    A.call("srcdsp_fill_synthetic", _ptr(t), k, n, seed, channel, offset, lo, hi, _stream(t))
    return t


# ================================================================ FIFO (8f.3)
class FifoWithTimeTrack(_Handle):
    """dsptl::FifoWithTimeTrack<T, N> (buffers.h:58-459) with its N-element
    ring in HBM.  T is a numpy dtype (e.g. np.dtype(("<i2", 2)) for
    complex<int16_t>, np.float64, np.complex64).  write() takes host (numpy,
    staged through double-buffered pinned memory) or device (torch) input;
    read() returns (error, start, out) -- the reference's bool, its start
    after the call (raised to timeStart when it asked for older samples), and
    the values (device tensor when `out` is one, else numpy)."""

    _destroy = "srcdsp_fifo_destroy"

    def __init__(self, dtype, N: int, samplingFrequency: float = 0.0):
        self.dtype, self.N = np.dtype(dtype), int(N)
        self._h = C.c_void_p()
        A.call("srcdsp_fifo_create", C.byref(self._h), self.dtype.itemsize, self.N, float(samplingFrequency))

    def _count_elems(self, x) -> int:
        nb = x.numel() * x.element_size() if _is_device(x) else np.asarray(x).nbytes
        if nb % self.dtype.itemsize:
            raise ValueError("buffer is not a whole number of FIFO elements")
        return nb // self.dtype.itemsize

    def write(self, inp, seconds: int = 0, fracSeconds: float = 0.0):
        n = self._count_elems(inp)
        if _is_device(inp):
            A.call("srcdsp_fifo_write_device", self._h, _ptr(inp), n, int(seconds), float(fracSeconds), _stream(inp))
        else:
            x = np.ascontiguousarray(inp)  # raw element bytes (a subarray dtype would broadcast)
            A.call("srcdsp_fifo_write", self._h, C.c_void_p(x.ctypes.data), n, int(seconds), float(fracSeconds))

    def read(self, out, start: int):
        """out: an element count (host numpy result) or a buffer to fill."""
        if isinstance(out, (int, np.integer)):
            out = np.zeros(int(out), self.dtype)
        n = self._count_elems(out)
        st, err = C.c_uint64(int(start)), C.c_int(0)
        if _is_device(out):
            A.call("srcdsp_fifo_read", self._h, _ptr(out), n, C.byref(st), C.byref(err), _stream(out))
        else:
            A.call("srcdsp_fifo_read_host", self._h, C.c_void_p(out.ctypes.data), n, C.byref(st), C.byref(err))
        return bool(err.value), st.value, out

    def count(self) -> int:
        c = C.c_size_t()
        A.call("srcdsp_fifo_count", self._h, C.byref(c))
        return c.value

    def reset(self):
        A.call("srcdsp_fifo_reset", self._h)

    def state(self):
        """(writePtr, timeStart, timeEnd, rolloverFlag) -- what dumpInfo() prints."""
        wp, ts, te, ro = C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_int()
        A.call("srcdsp_fifo_get_state", self._h, C.byref(wp), C.byref(ts), C.byref(te), C.byref(ro))
        return wp.value, ts.value, te.value, bool(ro.value)

    def getAbsoluteTime(self, timePoint: int, fracTimePoint: float = 0.0):
        s, fs = C.c_uint(), C.c_double()
        A.call("srcdsp_fifo_get_absolute_time", self._h, int(timePoint), float(fracTimePoint), C.byref(s),
               C.byref(fs))
        return s.value, fs.value
