"""Python mirror of the device sampler's scripted-set draw (csrc/episode_stream.hpp, pcg64_choice_set), on top of
``PCG64.random_raw()`` with numpy's half-word buffering.  It restates, as a SET, what
``Generator.choice(n, size=k, replace=False)`` (p None, n <= 10000) does: Floyd's algorithm, then the shuffle's draws."""
import numpy as np


class Pcg64Mirror:
    """numpy's PCG64 as the kernels hold it: raw 64-bit outputs, next_uint32 keeps the upper half for the next call."""

    def __init__(self, seed):
        self.bitgen = np.random.PCG64(np.random.SeedSequence(seed))
        self.has32, self.half = 0, 0

    def next32(self) -> int:
        if self.has32:
            self.has32 = 0
            return self.half
        v = int(self.bitgen.random_raw())
        self.has32, self.half = 1, v >> 32
        return v & 0xFFFFFFFF

    def bounded(self, rng: int) -> int:
        """uniform in [0, rng], Lemire's multiply-shift with rejection; rng == 0 draws nothing (pcg64_bounded)."""
        if rng == 0:
            return 0
        excl = rng + 1
        m = self.next32() * excl
        left = m & 0xFFFFFFFF
        if left < excl:
            thr = (0xFFFFFFFF - rng) % excl
            while left < thr:
                m = self.next32() * excl
                left = m & 0xFFFFFFFF
        return m >> 32

    def choice_set(self, n: int, k: int) -> int:
        """The mask form: bit mask of choice(n, k, replace=False)."""
        mask = 0
        for j in range(n - k, n):
            v = self.bounded(j)
            mask |= 1 << (j if (mask >> v) & 1 else v)
        for i in range(k - 1, 0, -1):          # the shuffle of the k results: draws consumed, order irrelevant to a set
            self.bounded(i)
        return mask

    def state(self):
        """(128-bit state, has_uint32, uinteger) - what ``Generator.bit_generator.state`` reports."""
        return self.bitgen.state["state"]["state"], self.has32, self.half
