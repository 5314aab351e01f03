"""Seeded inputs shared by tests/test_boundary_host.py, tests/test_boundary.py and tools: targets g whose channels cover the masks a
distance transform can get wrong, and sigmoid-like predictions p in (0, 1).

Target channels (make() returns their names per (sample, channel)):
  empty    all 0                                        the degenerate map: zeros
  full     all 1                                        the other degenerate map: zeros
  corner   one voxel at the far corner (D-1, H-1, W-1)  the largest distances of the grid, across every word and tile
  faces    a box that touches the d = 0 and w = 0 faces
  two      two separated boxes, one ending at the last column
  soft     1 / (1 + exp((r - r0) / 2 + noise)) around the centre: values spread over (0, 1), none constructed to sit at 0.5
Predictions: sigmoid(4 (shifted target - 0.5) + noise), so P = p > 0.5 is the target moved by a few voxels plus speckle; on the empty
and full channels the noise is small and P is empty / full as well."""
import numpy as np

SEED = 20192
A = (2, 3, 37, 19, 70)            # two mask words, the last ragged; three 32-column tiles, the last partial; D > 32: a second trip; all odd
B = (1, 2, 3, 5, 7)
C = (1, 3, 9, 64, 64)             # exactly one full word
LAYOUT = {A: (("empty", "full", "corner"), ("faces", "two", "soft")), B: (("corner", "soft"),), C: (("full", "two", "soft"),)}
ALPHAS = (1, 2, 2.5)


def _channel(kind, dhw, rng):
    D, H, W = dhw
    g = np.zeros(dhw, dtype=np.float32)
    if kind == "full":
        g[:] = 1.0
    elif kind == "corner":
        g[D - 1, H - 1, W - 1] = 1.0
    elif kind == "faces":
        g[:max(1, D // 3), H // 4:max(H // 4 + 1, H // 2), :max(1, W // 3)] = 1.0
    elif kind == "two":
        g[D // 4:max(D // 4 + 1, D // 2), :max(1, H // 3), W // 8:max(W // 8 + 1, W // 4)] = 1.0
        g[D - max(1, D // 4):, H - max(1, H // 3):, W - max(1, W // 5):] = 1.0
    elif kind == "soft":
        d, h, w = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        r = np.sqrt((d - D / 2.0) ** 2 + (h - H / 2.0) ** 2 + (w - W / 2.0) ** 2)
        g = (1.0 / (1.0 + np.exp((r - min(dhw) / 2.5) / 2.0 + rng.normal(0.0, 0.7, size=dhw)))).astype(np.float32)
    else:
        assert kind == "empty"
    return g


def make(shape, seed=SEED):
    """-> p, g float32 of `shape`, names: the kind of each target channel as LAYOUT[shape][n][c]"""
    rng = np.random.default_rng(seed)
    names = LAYOUT[shape]
    dhw = shape[2:]
    g = np.stack([np.stack([_channel(k, dhw, rng) for k in row]) for row in names]).astype(np.float32)
    shifted = np.roll(g, (2, 1, 3), axis=(2, 3, 4))
    sd = np.asarray([[0.3 if k in ("empty", "full") else 1.5 for k in row] for row in names]).reshape(shape[:2] + (1, 1, 1))
    p = (1.0 / (1.0 + np.exp(-(4.0 * (shifted - 0.5) + sd * rng.normal(size=shape))))).astype(np.float32)
    assert g.shape == tuple(shape) and 0.0 < p.min() and p.max() < 1.0
    return p, g, names


def hard(g):
    return (g > np.float32(0.5)).astype(np.float32)
