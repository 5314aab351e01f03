"""Seeded inputs shared by tests/test_lesion_loss_host.py, tests/test_lesion_loss.py, tests/lesion_loss_dp_worker.py and tools: targets
whose channels hold the lesions a labelling, a dilation or a per-lesion sum can get wrong, and sigmoid-like predictions p in (0, 1).

A target channel is the union of the kinds named for it, joined by "+" (LAYOUT[shape][n][c]):
  empty     all 0: a pair without a lesion
  full      all 1: one lesion, no background
  corner    one voxel at the far corner (D-1, H-1, W-1)
  faces     a box that touches the d = 0 and w = 0 faces
  diag      two voxels that touch only at a corner: 26-connected, one lesion at dilation 0
  straddle  two boxes 5 voxels apart along w, the gap across the boundary between the first two mask words (w = 58..61 and 67..70):
            two lesions at dilation <= 2, one at dilation 3
  far       two boxes in opposite corners of the grid
  speckle   rng.random < 0.03: hundreds of lesions, most of one voxel
  balls     3..8 balls of radius U(0.8, 3.5) at uniform centres
  soft      `balls`, box-filtered 2 x 2 x 2: values in {0, 1/8, ..., 1}
Predictions as in tests/boundary_inputs.py: sigmoid(4 (shifted target - 0.5) + noise)."""
import numpy as np

SEED = 20195
A = (2, 3, 17, 19, 37)            # all odd, a ragged mask word, W < 64
B = (1, 2, 3, 5, 7)               # tiny
C = (1, 3, 9, 64, 64)             # exactly one full word
D = (1, 2, 5, 6, 130)             # three words, the last ragged: dilation carries across words
LAYOUT = {A: (("corner+faces+diag", "speckle", "empty"), ("full", "far+diag", "soft")),
          B: (("corner+diag", "faces"),),
          C: (("full", "far+corner", "speckle"),),
          D: (("straddle+corner", "speckle+faces"),)}
SHAPES = {"A": A, "B": B, "C": C, "D": D}


def balls(dhw, rng, count=None):
    D_, H, W = dhw
    d, h, w = np.meshgrid(np.arange(D_), np.arange(H), np.arange(W), indexing="ij")
    g = np.zeros(dhw, dtype=bool)
    for _ in range(int(rng.integers(3, 9)) if count is None else count):
        c = rng.uniform(0, 1, size=3) * np.asarray(dhw)
        r = rng.uniform(0.8, 3.5)
        g |= (d - c[0]) ** 2 + (h - c[1]) ** 2 + (w - c[2]) ** 2 <= r * r
    return g


def box_filter(m):
    """the mean of the 2 x 2 x 2 block that starts at each voxel (zeros beyond the grid)"""
    x = np.pad(m.astype(np.float64), ((0, 1), (0, 1), (0, 1)))
    s = sum(x[a:a + m.shape[0], b:b + m.shape[1], c:c + m.shape[2]] for a in (0, 1) for b in (0, 1) for c in (0, 1))
    return (s / 8.0).astype(np.float32)


def _kind(kind, dhw, rng):
    D_, H, W = dhw
    g = np.zeros(dhw, dtype=np.float32)
    if kind == "full":
        g[:] = 1.0
    elif kind == "corner":
        g[D_ - 1, H - 1, W - 1] = 1.0
    elif kind == "faces":
        g[:max(1, D_ // 3), H // 4:max(H // 4 + 1, H // 2), :max(1, W // 3)] = 1.0
    elif kind == "diag":
        g[D_ // 2, H // 2, W // 2] = 1.0
        g[D_ // 2 + 1, H // 2 + 1, W // 2 + 1] = 1.0
    elif kind == "straddle":
        assert W >= 72
        g[1:3, 1:4, 58:62] = 1.0
        g[1:3, 1:4, 67:71] = 1.0
    elif kind == "far":
        g[:2, :3, 2:6] = 1.0
        g[D_ - 2:, H - 3:, W - 6:W - 2] = 1.0
    elif kind == "speckle":
        g = (rng.random(dhw) < 0.03).astype(np.float32)
    elif kind == "balls":
        g = balls(dhw, rng).astype(np.float32)
    elif kind == "soft":
        g = box_filter(balls(dhw, rng))
    else:
        assert kind == "empty", kind
    return g


def channel(kinds, dhw, rng):
    return np.maximum.reduce([_kind(k, dhw, rng) for k in kinds.split("+")])


def predict(g, rng, sd=1.5):
    """the target moved by (2, 1, 3) voxels through a sigmoid, plus noise"""
    shifted = np.roll(g, (2, 1, 3), axis=(2, 3, 4))
    p = (1.0 / (1.0 + np.exp(-(4.0 * (shifted - 0.5) + sd * rng.normal(size=g.shape))))).astype(np.float32)
    assert 0.0 < p.min() and p.max() < 1.0
    return p


def make(shape, seed=SEED):
    """-> p, g float32 of `shape`, names = LAYOUT[shape]"""
    rng = np.random.default_rng(seed)
    names = LAYOUT[shape]
    g = np.stack([np.stack([channel(k, shape[2:], rng) for k in row]) for row in names]).astype(np.float32)
    assert g.shape == tuple(shape)
    return predict(g, rng), g, names


def blob_targets(n, dhw, seed, empty=()):
    """[n, 3, D, H, W] hard targets for the Trainer runs: per channel four boxes in four octants of the grid, each moved by a few seeded
    voxels -- at least 3 separate lesions at dilation 1 -- except the (sample, channel) pairs listed in `empty`, which hold none."""
    rng = np.random.default_rng(seed)
    D_, H, W = dhw
    g = np.zeros((n, 3) + tuple(dhw), dtype=np.float32)
    octants = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]
    for i in range(n):
        for c in range(3):
            if (i, c) in empty:
                continue
            for o in octants:
                lo = [o[a] * (dhw[a] // 2) + 3 + int(rng.integers(0, 3)) for a in range(3)]
                size = [2 + int(rng.integers(0, 3 + c)) for _ in range(3)]
                g[i, c, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = 1.0
    return g
