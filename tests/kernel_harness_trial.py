"""Helper module of the kernel test of the trial snapshot (not collected by pytest): the call of
tests/kernels/harness_trial.cpp (through tests/kernel_harness.py) and the image a case is laid out in.

One image of bytes holds every source and every destination of a table.  A region starts at a 16-byte-aligned offset; the 8 bytes
before it and the 8 bytes right behind its last byte (not behind its last 16-byte unit: a store that rounds a tail up would hit
them) are canaries, and so is everything else that is no source: the whole image starts as a fixed pseudo-random background.  The
expected image after a launch is the image before it with every destination's bytes replaced by its source's -- compared whole, so
the canaries, the sources and the gaps are all covered by one comparison."""
from __future__ import annotations

import ctypes as C

import numpy as np

import kernel_harness as kh

UNIT = 16
CANARY = 8
MAX_SEGMENTS = 32                        # kTrialMaxSegments


def grid_units():
    """16-byte units one workgroup per 256 covers before the grid is capped."""
    return kh.load().rkt_grid() * 256


class Case:
    """`lengths`: the byte count of every segment.  Sources first, then destinations, each between its canaries."""

    def __init__(self, lengths, seed=0):
        self.lengths = np.asarray(lengths, dtype=np.int64)
        cursor, offsets = UNIT, []
        for _ in range(2):
            for n in self.lengths:
                cursor = (cursor + CANARY + UNIT - 1) // UNIT * UNIT      # at least 8 bytes of canary before the region
                offsets.append(cursor)
                cursor += int(n) + CANARY
        self.size = (cursor + UNIT - 1) // UNIT * UNIT + UNIT
        k = len(self.lengths)
        self.src, self.dst = np.array(offsets[:k], dtype=np.int64), np.array(offsets[k:], dtype=np.int64)
        rng = np.random.default_rng(seed)
        self.image = rng.integers(0, 256, self.size, dtype=np.uint8)

    def units(self):
        return int((self.lengths // UNIT).sum())

    def launch(self, image, src, dst):
        """The image after one launch src -> dst, and what it has to be."""
        want = image.copy()
        for s, d, n in zip(src, dst, self.lengths):
            want[d:d + n] = image[s:s + n]
        got = np.ascontiguousarray(image.copy())
        assert kh.load().rkt_max_segments() == MAX_SEGMENTS
        kh.invoke("rkt_trial_copy", C.c_void_p(got.ctypes.data), C.c_int64(got.size), C.c_int64(len(self.lengths)),
                  *(C.c_void_p(a.ctypes.data) for a in (src, dst, self.lengths)))
        return got, want


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else f"{bad.size} bytes differ, the first at offset {int(bad[0])} (got {int(got[bad[0]])}, want {int(want[bad[0]])})"
