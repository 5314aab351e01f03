"""Shared case builders of the CarveMix tests (tests/test_carvemix_host.py on the CPU, tests/test_carvemix.py on the device): seeded numpy, float32
data with a NaN and a -0.0 planted in donor and receiver alike.  A case is a dict: name, data [N,C,D,H,W], target [N,3,D,H,W], donor_data
[K,C,D,H,W], donor_target [K,3,D,H,W], u [K], side [K], dst (list or None), kinds [K] (the donors' target kinds), offset8 (the device tensors are
to be views 8 bytes off a 16-byte boundary).  `cases()` is the one list both files walk."""
import zlib

import numpy as np

SHAPE_A, SHAPE_B, SHAPE_C = (17, 19, 37), (3, 5, 7), (9, 64, 64)
US = (0.0, 0.3, 0.75, 1.0 - 2.0 ** -53)
DRAWS = tuple((u, side) for side in ("outer", "inner") for u in US)
DEGENERATE = ("empty", "full")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _ball(shape, centre, radius):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return sum((a - c) ** 2 for a, c in zip(g, centre)) <= radius * radius


# per shape: the balls (centre, radius), the box touching two faces, the single voxel
GEOMETRY = {
    SHAPE_A: dict(ball=((8, 9, 18), 5.0), two=(((5, 6, 8), 4.0), ((11, 12, 27), 3.0)), box=((0, 6), (0, 7), (10, 20)), single=(7, 3, 30)),
    SHAPE_B: dict(ball=((1, 2, 3), 1.0), two=(((1, 1, 1), 1.0), ((1, 3, 5), 1.0)), box=((0, 2), (0, 2), (0, 3)), single=(1, 2, 4)),
    SHAPE_C: dict(ball=((4, 30, 30), 3.5), two=(((4, 20, 17), 3.0), ((5, 41, 50), 2.5)), box=((0, 5), (20, 29), (0, 9)), single=(8, 63, 1)),
}


def donor_wt(kind, shape, seed=0):
    """the WT channel [D,H,W] float32 of a donor target of `kind`"""
    geo = GEOMETRY[shape]
    wt = np.zeros(shape, np.float32)
    if kind == "ball":
        wt[_ball(shape, *geo["ball"])] = 1.0
    elif kind == "two":
        for c, r in geo["two"]:
            wt[_ball(shape, c, r)] = 1.0
    elif kind == "box":
        wt[tuple(slice(a, b) for a, b in geo["box"])] = 1.0
    elif kind == "single":
        wt[geo["single"]] = 1.0
    elif kind == "soft":                                      # a teacher's probabilities around 0.5: solid core, noisy rim, exact 0.5 outside the mask
        c, r = geo["ball"]
        g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
        dist = np.sqrt(sum((a - b) ** 2 for a, b in zip(g, c)))
        wt = (0.5 + 0.4 * (1.0 - dist / r) + 0.04 * (_rng("soft", shape, seed).random(shape) - 0.5)).clip(0.0, 1.0).astype(np.float32)
        wt[0, 0, 0] = 0.5                                     # not above 0.5f: outside
        wt[-1, -1, -1] = np.float32(0.5)
    elif kind == "full":
        wt[...] = 1.0
    elif kind != "empty":
        raise ValueError(kind)
    return wt


def _plant(x, seed):
    """a NaN and a -0.0 at two seeded voxels of every leading index, one more of each at the first and the centre voxel of item 0"""
    r = _rng("plant", x.shape, seed)
    sp = x.shape[2:]
    n = int(np.prod(sp))
    at = lambda v: np.unravel_index(int(v), sp)               # x may be a strided view: written through, never reshaped
    for i in range(x.shape[0]):
        for c in range(x.shape[1]):
            a, b = r.choice(n, size=2, replace=False)
            x[i, c][at(a)] = np.nan
            x[i, c][at(b)] = -0.0
    x[0, 0][at(0)] = np.nan
    x[0, -1][at(n // 2)] = -0.0
    x[0, 0][at(n // 2)] = np.nan
    return x


def make_case(name, shape, n, c, kinds, draws, dst, offset8=False):
    k = len(kinds)
    r = _rng("case", name)
    data = _plant(r.standard_normal((n, c) + shape).astype(np.float32), 1)
    donor_data = _plant(r.standard_normal((k, c) + shape).astype(np.float32), 2)
    target = (r.random((n, 3) + shape) > 0.6).astype(np.float32)
    donor_target = np.zeros((k, 3) + shape, np.float32)
    for j, kind in enumerate(kinds):
        wt = donor_wt(kind, shape, seed=j)
        donor_target[j, 0] = wt
        donor_target[j, 1] = wt * (r.random(shape) > 0.3)
        donor_target[j, 2] = wt * (r.random(shape) > 0.6)
    _plant(donor_target[:, 1:], 3)                            # the select moves target words too
    _plant(target[:, 1:], 4)
    return dict(name=name, data=data, target=target, donor_data=donor_data, donor_target=donor_target, u=[d[0] for d in draws],
                side=[d[1] for d in draws], dst=dst, kinds=tuple(kinds), offset8=offset8)


def cases():
    out = []
    m = len(DRAWS)
    # (2, 4) at 17 x 19 x 37 (an odd voxel count: one by one), K = N with a permuted dst; donor 1 takes the draw five places on, so every kind
    # meets every u and both sides
    for pair in (("ball", "two"), ("box", "single"), ("soft", "empty"), ("full", "ball")):
        for i in range(m):
            out.append(make_case("A-%s-%s-%d" % (pair + (i,)), SHAPE_A, 2, 4, pair, (DRAWS[i], DRAWS[(i + 5) % m]), [1, 0]))
    # K < N with dst = [1]
    for i in (1, 6):
        out.append(make_case("A-ball-into-1-%d" % i, SHAPE_A, 2, 4, ("ball",), (DRAWS[i],), [1]))
    # (1, 4) at 3 x 5 x 7
    for kind in ("single", "box", "empty", "full"):
        for i in range(m):
            out.append(make_case("B-%s-%d" % (kind, i), SHAPE_B, 1, 4, (kind,), (DRAWS[i],), None))
    # (1, 1) at 9 x 64 x 64: the 16-byte lanes
    for kind in ("ball", "two", "box", "soft", "single", "empty", "full"):
        for i in range(m):
            out.append(make_case("C-%s-%d" % (kind, i), SHAPE_C, 1, 1, (kind,), (DRAWS[i],), None))
    # tensors 8 bytes off a 16-byte boundary: the map is not, so the pair goes one by one (the count of the threshold call keeps its lanes)
    for i in (2, 7):
        out.append(make_case("C-off8-two-%d" % i, SHAPE_C, 1, 1, ("two",), (DRAWS[i],), None, offset8=True))
        out.append(make_case("A-off8-ball-%d" % i, SHAPE_A, 2, 4, ("ball",), (DRAWS[i],), [1], offset8=True))
    return out


def words(a):
    """the int32 view that equality is taken on: NaN payloads and the sign of zero count"""
    return np.ascontiguousarray(a).view(np.int32)
