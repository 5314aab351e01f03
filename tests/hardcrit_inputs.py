"""Seeded inputs shared by tests/test_hardcrit_host.py and tests/test_hardcrit.py: p = sigmoid(N(0, 2.5)) as float32, g = Bernoulli(0.3)."""
import numpy as np

SEED = 20191
ODD = (2, 3, 17, 19, 37)          # V = 11951 is odd: rows start off a 16-byte boundary, end in a partial quad and span two moments chunks
TINY = (1, 1, 1, 1, 5)            # fewer elements than two quads; K = 1
TWO_TRIPS = (1, 3, 64, 96, 128)   # 2,359,296 elements: more than one trip of 2048 workgroups x 256 lanes x 4 floats
KS = (0.001, 1, 10, 50, 100)
BG_WEIGHTS = (1, 1e-2)
BAND = 1e-4                       # elements whose float64 l lies within t * (1 +- BAND) may fall on either side of a float32 threshold
BAND_CAP = 16


def make(shape, seed=SEED):
    rng = np.random.default_rng(seed)
    p = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.5, size=shape)))).astype(np.float32)
    g = (rng.random(size=shape) < 0.3).astype(np.float32)
    return p, g


def make_ties(shape=(1, 2, 7, 9, 11), seed=SEED + 1):
    """p quantised to {0.1, 0.5, 0.9}, binary g: l takes six distinct values (bg_weight 1: three, each shared by two (p, g) classes)"""
    rng = np.random.default_rng(seed)
    p = rng.choice(np.asarray([0.1, 0.5, 0.9], dtype=np.float32), size=shape)
    g = (rng.random(size=shape) < 0.3).astype(np.float32)
    return p, g
