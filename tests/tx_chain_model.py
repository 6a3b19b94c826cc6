"""One transmit chain stepped call by call on the CPU: the yardstick of the
fused transmit families (srcdsp_upmix_*, srcdsp_modulate_*,
srcdsp_modulate_offset_*).  It generalises stagger_model.offset_chain and is
composed only of pieces the suite pins to the reference:

    UPMIX            samples ->          oracle up ->            oracle mixer
    MODULATE         bits -> MapperModel -> oracle up ->         oracle mixer
    MODULATE_OFFSET  bits -> MapperModel -> oracle up -> StaggerModel -> oracle mixer

(tests/test_tx_chain_model.py replays the chain goldens recorded from the
reference build through it).  After every step the whole state can be read,
and the chain can be copied.

The oracle's handles have no copy of their own, so a copy is rebuilt from what
fixes the state: an interpolator's history is its last H - 1 inputs (zeros
after a reset, the flush's zeros included), a mixer's (phase, word, nominal
frequency) follow from its calls since the last reset and the number of
samples stepped between them, whatever the samples were."""
from __future__ import annotations

import numpy as np

from mapper_model import QPSK, MapperModel
from stagger_model import StaggerModel

UPMIX, MODULATE, MODULATE_OFFSET = "upmix", "modulate", "modulate_offset"
FAMILIES = (UPMIX, MODULATE, MODULATE_OFFSET)


class _Up:
    """The oracle's interpolator with the inputs that make up its history."""

    def __init__(self, o, variant, L, taps, tail=None):
        self.o, self.variant, self.L = o, variant, L
        self.taps = np.array(taps)
        self.H = len(self.taps) // L
        self.up = o.up(variant, L, self.taps)
        self.tail = np.zeros((max(self.H - 1, 0), 2), np.int16)
        if tail is not None and len(tail):
            self.up.step(tail)  # the outputs are dropped: only the history is wanted
            self.tail = np.array(tail, np.int16)

    @property
    def length(self):
        return self.up.length

    def copy(self):
        return _Up(self.o, self.variant, self.L, self.taps, self.tail)

    def reset(self):
        self.up.reset()
        self.tail[:] = 0

    def step(self, x, flush, iterator):
        x = np.ascontiguousarray(x, np.int16).reshape(-1, 2)
        y = np.asarray(self.up.step(x, flush, iterator)).reshape(-1, 2)
        zeros = np.zeros((self.length // self.L if flush else 0, 2), np.int16)  # what a flush feeds
        fed = np.concatenate([self.tail, x, zeros])
        self.tail = fed[len(fed) - (self.H - 1):].copy()
        return y


class _Mixer:
    """The oracle's mixer with the calls that lead to its state."""

    def __init__(self, o, N, log=()):
        self.o, self.N = o, N
        self.m = o.mixer(N)
        self.log = []
        for op, v in log:
            getattr(self, op)(v)

    def copy(self):
        return _Mixer(self.o, self.N, self.log)

    def reset(self, f):
        self.m.reset(f)
        self.log = [("reset", f)]

    def set_frequency(self, f):
        self.m.set_frequency(f)
        self.log.append(("set_frequency", f))

    def adjust_frequency(self, f):
        self.m.adjust_frequency(f)
        self.log.append(("adjust_frequency", f))

    def advance(self, n):
        """n samples, whatever they are."""
        self.step(np.zeros((n, 2), np.int16))

    def step(self, x):
        y = np.asarray(self.m.step(x)).reshape(-1, 2)
        if len(x):
            if self.log and self.log[-1][0] == "advance":
                self.log[-1] = ("advance", self.log[-1][1] + len(x))
            else:
                self.log.append(("advance", len(x)))
        return y

    def state(self):
        return tuple(self.m.state()[:2])


class TxChain:
    """family: UPMIX (step takes samples, int16 [n, 2]) or MODULATE /
    MODULATE_OFFSET (step takes bits, uint8 [n]; kind is mapper_model.SDPSK or
    QPSK, D the stagger's delay of the offset family)."""

    def __init__(self, o, family, L, taps, N=4096, freq=0.0, kind=None, D=None, variant=0, mapper_state=0):
        assert family in FAMILIES
        self.family = family
        self.mapper = MapperModel(kind, mapper_state) if family != UPMIX else None
        self.up = _Up(o, variant, L, taps)
        self.stagger = StaggerModel(D) if family == MODULATE_OFFSET else None
        self.mixer = _Mixer(o, N)
        self.mixer.reset(freq)

    def copy(self):
        c = object.__new__(TxChain)
        c.family = self.family
        c.mapper = MapperModel(self.mapper.kind, self.mapper.state) if self.mapper else None
        c.up = self.up.copy()
        c.stagger = self.stagger.copy() if self.stagger else None
        c.mixer = self.mixer.copy()
        return c

    __copy__ = copy

    @property
    def L(self):
        return self.up.L

    def n_sym(self, n):
        """Interpolator inputs of a step of n samples / bits."""
        return self.mapper.n_out(n) if self.mapper else n

    def n_out(self, n, flush=False):
        return self.L * (self.n_sym(n) + (self.up.length // self.L if flush else 0))

    def step(self, x, flush=False, iterator=False) -> np.ndarray:
        y = self.mapper.step(x) if self.mapper else np.ascontiguousarray(x, np.int16).reshape(-1, 2)
        y = self.up.step(y, flush, iterator)
        if self.stagger:
            y = self.stagger.step(y)
        return self.mixer.step(y)

    def state(self) -> dict:
        """What the handles report; the interpolator's history shows in a
        further step (of a copy)."""
        s = {"mixer": self.mixer.state()}
        if self.mapper:
            s["mapper"] = self.mapper.state
        if self.stagger:
            s["carry"] = self.stagger.carry.tolist()
        return s

    # what may happen between two steps
    def set_frequency(self, f):
        self.mixer.set_frequency(f)

    def adjust_frequency(self, f):
        self.mixer.adjust_frequency(f)

    def reset_mixer(self, f=0.0):
        self.mixer.reset(f)

    def reset_mapper(self):
        self.mapper.reset()

    def set_mapper_state(self, s):
        self.mapper.state = int(s)

    def reset_stagger(self):
        self.stagger.reset()

    def reset_up(self):
        self.up.reset()
