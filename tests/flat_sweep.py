"""What tests/test_optim_recipe.py, tests/test_flat_passes.py and tests/test_hardcrit_host.py share for the flat streaming passes
(csrc/flat_lanes.hpp): a run of elements between guards on the device, the lengths and alignments of the sweep, and its seeded inputs."""
import ctypes as C
import functools

import numpy as np

import hardcrit_inputs as I

NS = [1, 3, 4, 5, 255, 1027, 4099, (1 << 21) + 4099]         # the last is past one sweep of the 2048-workgroup grid (2048 * 256 lanes * 4 floats = 2^21)
OFFSETS = [0, 1, 2, 3]
SWEEP = [(n, off) for n in NS for off in OFFSETS if n < (1 << 21) or off in (0, 3)]
MIXED_N = 4099                                               # the length of the cases whose pointers sit at different offsets
PAD = 4                                                      # guard elements on either side of a run
GUARDS = {np.dtype(np.float32): -12345.0, np.dtype(np.int32): -12345, np.dtype(np.uint32): 0xFFFFCFC7}


class Slab:
    """a run of n float32 / int32 / uint32 elements at element offset `off` from a 16-byte boundary, PAD guard elements before it and
    PAD + (4 - off) after"""

    def __init__(self, values, off):
        import torch
        values = np.asarray(values)
        self.dtype, self.n, self.lo = values.dtype, len(values), PAD + off
        host = np.full(self.lo + self.n + PAD + 4, GUARDS[self.dtype], dtype=self.dtype)
        host[self.lo:self.lo + self.n] = values
        self.t = torch.from_numpy(host.view(np.float32 if self.dtype == np.float32 else np.int32)).cuda()     # 32 bits are 32 bits
        assert self.t.data_ptr() % 16 == 0
        self.ptr = C.c_void_p(self.t.data_ptr() + 4 * self.lo)

    def get(self):
        h = self.t.cpu().numpy().view(self.dtype)
        guard = h.dtype.type(GUARDS[self.dtype])
        assert np.all(h[:self.lo] == guard) and np.all(h[self.lo + self.n:] == guard), "a kernel wrote outside its run"
        return h[self.lo:self.lo + self.n].copy()


def seed(n, off):
    return I.SEED + 1000 * n + off


@functools.lru_cache(maxsize=None)
def probabilities(n, off):
    """(p, g) of hardcrit_inputs.make for a run of n elements, one seed per (n, off)"""
    return I.make((n,), seed=seed(n, off))


@functools.lru_cache(maxsize=None)
def distance_maps(n, off):
    """two int32 runs in [-2^18, 2^18] with about a tenth of the values exactly 0: what the passes read of a signed squared distance map"""
    rng = np.random.default_rng(seed(n, off) + 500)
    maps = rng.integers(-(1 << 18), (1 << 18) + 1, size=(2, n)).astype(np.int32)
    maps[rng.random(size=(2, n)) < 0.1] = 0
    return maps[0], maps[1]


def topk_case(n, off):
    """(K, k in per cent, bg_weight) of the sweep's top-k case: K = max(1, n // 10), the background weight alternates with the offset"""
    return max(1, n // 10), 10.0, I.BG_WEIGHTS[off % 2]
