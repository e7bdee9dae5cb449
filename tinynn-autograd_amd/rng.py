"""The device random generator: a counter-based Philox4x32-10 stream (dropout.py states it exactly) whose state
{uint64 seed, uint64 calls} lives in HBM, so a draw is capturable into a hipGraph, reproducible from a seed and exactly
predictable on the host.

    g = Generator(1234)            or the module default: manual_seed(1234)
    u = g.uniform((4, 8))          a device fill: ONE ticket launch and ONE data launch, no host draw, no upload
    g.state()                      (seed, calls) — with the native library a read-back and a synchronisation

With the native library (include/tnn_dropout.h) the state is a 16-byte device array that only kernels advance: every drawing
call — Generator.uniform, device_array.dropout — consumes one value of `calls`.  Under the CPU test twin, which has none of
the entry points, the state is two host integers and the numbers come from dropout.py's numpy generator; the stream is the
same either way.

Nothing here touches numpy's global RNG (utils/seeder.py): the shuffles and the parameter draws of a seeded run consume
exactly the numbers they did before.
"""

import numpy as np

from . import _lib
from . import device_array as da
from . import dropout as _dp

_MASK64 = (1 << 64) - 1


class Generator(object):
    """One stream of random numbers.  The device state is allocated at the first native draw (or `state()`), so creating and
    seeding a generator touches no device; inside an open graph capture a generator must already have its state (draw or
    seed-and-read once before: tn.capture's warm-up calls do)."""

    def __init__(self, seed=0):
        self._seed, self._calls, self._dev = int(seed) & _MASK64, 0, None

    @staticmethod
    def native():
        return _lib.get().has_dropout

    # ------------------------------------------------------------------ state
    def manual_seed(self, seed):
        """{seed, calls = 0}; returns the generator."""
        return self.set_state(seed, 0)

    def set_state(self, seed, calls):
        self._seed, self._calls = int(seed) & _MASK64, int(calls) & _MASK64
        if self._dev is not None:
            _lib.get().rng_set(self._dev._ptr, self._seed, self._calls)      # a one-thread launch, in stream order
        return self

    def state(self):
        """(seed, calls).  With a device state: a read-back, which synchronises (and cannot run inside a capture)."""
        if self._dev is not None:
            seed, calls = (int(v) & _MASK64 for v in np.asarray(self._dev))
            self._seed, self._calls = seed, calls
        return self._seed, self._calls

    def device_state(self):
        """The 16-byte device record {seed, calls} (native library only), allocated and written on first use."""
        if self._dev is None:
            if _lib.capturing:
                raise RuntimeError("rng.Generator: the device state would be allocated inside an open graph capture — draw "
                                   "from the generator (or call device_state()) once before capturing")
            dev = da.DeviceArray._new((2,), np.int64)
            _lib.get().rng_set(dev._ptr, self._seed, self._calls)
            self._dev = dev
        return self._dev

    def advance(self, seed, calls):
        """The composed route's bookkeeping after it drew with the ticket (seed, calls): the state becomes (seed, calls + 1)."""
        return self.set_state(seed, (calls + 1) & _MASK64)

    # ------------------------------------------------------------------ draws
    def uniform(self, shape, dtype=None, first=0):
        """Uniform numbers in [0, 1) — r 2^-24 of the 24-bit draws, exact — as a device array of `shape`; consumes one call.
        float32 (default float) or float64.  first: the stream index of element 0."""
        dtype = np.dtype(da.get_default_float() if dtype is None else dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("Generator.uniform: float32 or float64, got %s" % dtype.name)
        shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(s) for s in shape)
        first, n = _dp.check_stream(first, int(np.prod(shape, dtype=np.int64)))
        if self.native():
            state = self.device_state()
            ticket = da.DeviceArray._new((2,), np.int64)
            out = da.DeviceArray._new(shape, dtype)
            _lib.get().rng_uniform(state._ptr, ticket._ptr, out._ptr, first, n, out._code())
            return out
        seed, calls = self.state()
        out = da.asarray(_dp.uniform(seed, calls, first, n, dtype).reshape(shape), dtype=dtype)
        self.advance(seed, calls)
        return out


default_generator = Generator(0)


def manual_seed(seed):
    """Seed the module's default generator (what dropout layers and ops draw from when they are given none)."""
    return default_generator.manual_seed(seed)


def state():
    return default_generator.state()


def uniform(shape, dtype=None):
    return default_generator.uniform(shape, dtype)
