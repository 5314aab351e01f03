"""Seeded cases and float64 restatements shared by tests/test_gather_host.py (no GPU) and tests/test_gather.py (the kernels): the eight-corner gathers
that cut every training patch -- `zoom_voxel` / `affine_voxel` (csrc/augment_voxel.hpp) behind ru_augment_patch[_soft], ru_augment_patch_affine and
ru_augment_batch_packed, and `elastic_warp_kernel` (csrc/elastic.hip) behind ru_elastic_warp.  Plain numpy.

WHAT THE RESTATEMENTS DEFINE.  Per axis a gather has two cells (i0, i0 + 1), a weight t of the upper cell and 1 - t of the lower one.
  zoom    x = fl64(index * scale), i0 = floor(x); t = float32(index * scale - i0) with the product EXACT (the kernel's fma(scale, index, -floor)),
          rounded once.  Where fl64 rounds the product up to an integer the exact difference is a NEGATIVE number near -4.4e-16 (index 10 at scale
          0.7: 10 * 0.7 -> 7.0; at 0.9 it rounds down and leaves +2.2e-16), and that is the weight: the data are unaffected at float32, but a hard
          target -- a sum of weights -- is then a negative number of that size where scipy gives 0.  By design: every consumer in csrc/ thresholds
          targets at 0.5.  Cells are reflected
          into the crop on the half-sample-symmetric extension (d c b a | a b c d | d c b a), periodic in 2 P.
  affine  s = ((m0 i + m1 j) + m2 k) + offset in float64, every operation rounded on its own, clamped to [-2, n] (NaN -> -2); i0 = floor(s),
          t = float32(s - i0); a cell outside the volume contributes raw 0 / label 0 / soft 0.
  warp    c = index + displacement in float64, 0 where not |c| < 1e9; i0 = floor(c), t = float32(c - i0), order 0 picks floor(c + 0.5); reflected.
t is float32 BY DEFINITION (both sides compute it from the same float64 coordinate), everything after it is float64 here: 1 - t, the three-factor
corner weights, the eight products and their sum, ((acc - mean) * inv_std) * gain + bias, WT = (1 + 2) + 3, TC = 1 + 3, ET = 3.

THE BARS are per voxel: the float32 roundings of `gather_corners` (and of the warp's corner loop), each allowed 2^-24 of the magnitude it acts on,
with S = sum_q |w_q| |x_q| over the eight corners:
  corner weights   1.f - t per axis and the product: 3 roundings per corner, each on |w_q x_q|                          ->  3 S
  fused adds       fmaf(w, x, acc), one rounding per corner on a partial sum that |.| bounds by S                       ->  8 S
  acc - mean       one rounding on at most S + |mean|;   (.) * inv_std   one more on the same, scaled                 ->  2 (S + |mean|)
  fmaf(z, gain, bias)   one rounding on the result                                                                      ->  |result|
  data bar = 2^-24 ((11 S + 2 (S + |mean|)) |inv_std gain| + |result|)
  soft targets: the data rule without the tail, 2^-24 * 11 S.   hard targets: sums of at most eight weights, S_k = sum of |w_q| over the corners of
  the channel's classes: 3 per weight + 8 adds + the class sums (2 for WT, 1 for TC, 0 for ET) -> 2^-24 * (13, 12, 11) S_k.
  warp: the corner loop `acc += w * x` carries no contraction pragma, so fused and unfused forms are both allowed: 3 S (weights) + S (the products)
  + 8 S (the adds), then acc * gain and + bias each on its own: 2^-24 (12 S |gain| + |acc gain| + |result|).  Order-0 targets: bar 0.
  Underflow: a rounding keeps 2^-24 of its result only down to float32's normal range; below it, it can lose up to 2^-149 outright (three tie
  weights of -4.4e-16 multiply to -8.7e-47, which float32 holds as 0).  Two products per corner weight act on |x_q|, eight adds on their own:
  every bar gains the floor 2^-149 (sum_q |x_q| + 8), carried through |inv_std gain| like S.  It is about 1e-39 for intensities of 65535.
In the EXACT family (integer intensities below 2^12, integer mean, power-of-two inv_std and gain, dyadic bias, soft values on the 2^-8 grid, scales,
matrices, offsets and displacements on the 0.25 grid) every weight, product and partial sum is exact in float32 and every bar is 0.

`run(case, mode="ref" | "emu", mutant=None)` evaluates a case: "ref" as above, "emu" in the kernels' float32 operation order (fmaf(w, x, acc) as
float32(float64(w) * float64(x) + float64(acc))), and `mutant` names one deliberate defect of MUTANTS."""
import functools

import numpy as np

SEED = 20196
U = 2.0 ** -24
TINY = 2.0 ** -149                     # float32's smallest subnormal: what a rounding can lose where a result underflows
DIMS = (19, 23, 37)
BIG = (100, 100, 124)
BIG_PATCH = (96, 96, 120)              # 1 105 920 voxels > 4096 blocks of 256: the zoom pass, the affine row mapping, a packed zoom-only launch
WARP_BIG = (128, 128, 132)             # 2 162 688 voxels > 8192 blocks of 256: the warp
CAP_ZOOM, CAP_WARP = 4096 * 256, 8192 * 256
SHAPES = ((1, 1, 1), (1, 9, 33), (9, 1, 7), (5, 7, 9))       # ragged against 256 threads and against the 4 x 4 x 16 brick tile
TIE_PATCH = (11, 12, 21)                                     # holds index 10 on every axis: the product ties of tests/test_resident.py
EXACT_SCALES = (0.25, 0.75, 1.0, 1.25, 2.5, 3.75)
REAL_SCALES = ((0.7, 1.0, 1.3), (1.3, 0.7, 1.0), (0.001, 2.5, 5.25), (5.25, 0.001, 2.5), (2.5, 5.25, 0.001))
TIE_SCALES = ((0.7, 0.9, 1.1), (1.3, 1.2, 0.7), (1.2, 1.3, 0.9))

BATCH_PATCH = (7, 7, 9)                                      # P0 == P1: a launch of more than one sample may transpose
# one ru_augment_batch_packed call each: more than RU_AUG_BATCH_MAX = 8 uint16 zoom samples (a zoom-only kernel, two launches); zoom and affine, uint16
# and float32 boxes, hard and soft targets in one launch (the kernel that holds all eight bodies), in the exact family with 9 samples and in the real one
BATCHES = {"u16 zoom x9": tuple("zoom real batch u16 %d" % i for i in range(9)),
           "exact mixed x9": tuple(("zoom" if i % 2 == 0 else "affine") + " exact batch mixed %d" % i for i in range(9)),
           "real mixed x9": tuple(("zoom" if i % 2 == 0 else "affine") + " real batch mixed %d" % i for i in range(9))}

MUTANTS = ("whole_sample_reflect", "reflect_no_period", "swap_weights", "swap_q", "flip_after_transpose", "drop_crop_lo", "tc_1_plus_2",
           "neighbour_gain", "neighbour_bias", "mean_before_fill", "clamp_to_edge", "trunc_not_floor", "round_half_even", "second_pass_repeats",
           "box_forgets_lo")


# ---------------------------------------------------------------------------------------------------------------- volumes
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def zscore_host(image):
    """(mean, std) float64 per channel, dataloader.zscore_stats' definition: the count is over x > 0, the sums over all voxels"""
    x = np.asarray(image, np.float64)
    n = (x > 0).sum(axis=(1, 2, 3)).astype(np.float64)
    mean = x.sum(axis=(1, 2, 3)) / n
    return mean, np.sqrt(np.square(x).sum(axis=(1, 2, 3)) / n - mean * mean)


@functools.lru_cache(maxsize=None)
def volume(name):
    """dict(image [4,D,H,W] float32, label [D,H,W] uint8 using all of 0..3, soft [3,D,H,W] float32, mean, istd float32 [4], box (lo, size), exact):
      exact        integers below 2^12 in a box with zeros around it, soft on the 2^-8 grid, integer mean, power-of-two inv_std
      exact_full   the same, the box is the whole volume (flush crops see values at all six faces)
      brats        integers 0..65535 in a box with zeros around it (a uint16 packed case), statistics of zscore_host
      frac         fractional and negative values, the box is the whole volume (a float32 packed case)
      big          100 x 100 x 124, two channels of `brats` kind: the two-pass shapes"""
    r = np.random.default_rng([SEED, sorted(("exact", "exact_full", "brats", "frac", "big")).index(name)])
    dims = BIG if name == "big" else DIMS
    c = 2 if name == "big" else 4
    if name in ("exact_full", "frac"):
        lo, size = (0, 0, 0), dims
    elif name == "big":
        lo, size = (4, 4, 4), (92, 92, 116)
    else:
        lo, size = (2, 3, 4), (14, 17, 28)
    sl = tuple(slice(a, a + n) for a, n in zip(lo, size))
    image = np.zeros((c,) + dims, np.float32)
    label = np.zeros(dims, np.uint8)
    soft = np.zeros((3,) + dims, np.float32)
    exact = name.startswith("exact")
    if exact:
        vals = r.integers(0, 4096, size=(c,) + size).astype(np.float32)
    elif name == "frac":
        vals = (r.integers(0, 65536, size=(c,) + size) * 0.37 - 900.0).astype(np.float32)
    else:
        vals = r.integers(0, 65536, size=(c,) + size).astype(np.float32)
        vals *= r.random((c,) + size) < 0.8                                   # zeros inside the tissue too
    vals[:, 0, 0, 0] = 1.0                                                    # both extreme corners are occupied: the box is [lo, lo + size) exactly
    vals[:, -1, -1, -1] = 4095.0 if exact else 65535.0
    image[(slice(None),) + sl] = vals
    inner = r.integers(0, 4, size=size).astype(np.uint8)
    label[sl] = inner
    if exact:
        soft[(slice(None),) + sl] = r.integers(0, 257, size=(3,) + size).astype(np.float32) / 256.0
        mean = np.array([512.0, 1024.0, 300.0, 7.0], np.float32)[:c]
        istd = np.array([2.0 ** -9, 2.0 ** -8, 2.0 ** -10, 2.0 ** -7], np.float32)[:c]
    else:
        soft[(slice(None),) + sl] = r.random((3,) + size).astype(np.float32)
        m, s = zscore_host(image)
        mean, istd = m.astype(np.float32), (1.0 / s).astype(np.float32)
    _frozen(image, label, soft, mean, istd)
    return dict(name=name, image=image, label=label, soft=soft, mean=mean, istd=istd, box=(lo, tuple(size)), dims=dims, exact=exact)


def _gain_bias(r, c, exact):
    if exact:
        return np.array([1.0, 2.0, 0.5, 4.0], np.float32)[:c], np.array([0.25, -0.5, 1.75, -3.0], np.float32)[:c]
    return r.uniform(0.9, 1.1, c).astype(np.float32), r.uniform(-0.2, 0.2, c).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- cases
def _zoom(name, vol, patch, lo, scale, flags=0, channels=4, soft=False, seed=0):
    v = volume(vol)
    gain, bias = _gain_bias(np.random.default_rng([SEED, 1, seed]), channels, v["exact"])
    return dict(name="zoom " + name, kind="zoom", family="exact" if v["exact"] else "real", vol=vol, patch=tuple(patch), lo=tuple(int(a) for a in lo),
                scale=tuple(float(s) for s in scale), flags=int(flags), C=channels, soft=bool(soft), gain=gain, bias=bias)


def _fit(r, dims, patch):
    return tuple(int(r.integers(0, d - p + 1)) for d, p in zip(dims, patch))


@functools.lru_cache(maxsize=None)
def zoom_cases():
    r = np.random.default_rng([SEED, 2])
    out = []
    for fam, vols in (("exact", ("exact", "exact_full")), ("real", ("brats", "frac"))):
        triples = [tuple(EXACT_SCALES[(a + b) % 6] for b in (0, 2, 5)) for a in range(6)] if fam == "exact" else list(REAL_SCALES)
        n = 0
        for si, patch in enumerate(SHAPES):
            for ti, scale in enumerate(triples):
                vol = vols[(si + ti) % 2]
                out.append(_zoom("%s %s s%d" % (fam, "x".join(map(str, patch)), ti), vol, patch, _fit(r, DIMS, patch), scale, flags=(5 * n + 3) % 16,
                                 soft=n % 3 == 2, seed=n))
                n += 1
        for ti, scale in enumerate(TIE_SCALES if fam == "real" else triples[:3]):             # index 10 at 0.7 / 0.9 / 1.1 / 1.3, index 5 at 1.2
            out.append(_zoom("%s ties s%d" % (fam, ti), vols[ti % 2], TIE_PATCH, _fit(r, DIMS, TIE_PATCH), scale, flags=(0, 7, 13)[ti], soft=ti == 1, seed=40 + ti))
        patch = SHAPES[3]
        far = tuple(d - p for d, p in zip(DIMS, patch))
        for fi, lo in enumerate(((0, 0, 0), far, (0, far[1], 0), (far[0], 0, far[2]))):       # flush with all six faces
            out.append(_zoom("%s flush %d" % (fam, fi), vols[1], patch, lo, triples[fi % len(triples)], flags=fi * 5, soft=fi == 3, seed=50 + fi))
        for flags in range(16):                                                              # flips and transpose on a non-square patch
            out.append(_zoom("%s flags %d" % (fam, flags), vols[flags % 2], patch, _fit(r, DIMS, patch), triples[flags % len(triples)], flags=flags,
                             soft=flags % 4 == 1, seed=60 + flags))
        for i in range(9):                                                                   # members of BATCHES: one patch, one channel count
            if fam == "real":                                                                # nine uint16 zoom samples, no transpose (P0 != P1): chunks of 8 + 1
                out.append(_zoom("real batch u16 %d" % i, "brats", SHAPES[3], _fit(r, DIMS, SHAPES[3]), (REAL_SCALES + TIE_SCALES)[i % 8], flags=i % 8, seed=150 + i))
            if i % 2 == 0:                                                                   # the zoom half of the mixed launches, P0 == P1
                out.append(_zoom("%s batch mixed %d" % (fam, i), vols[(i // 2) % 2], BATCH_PATCH, _fit(r, DIMS, BATCH_PATCH), triples[i % len(triples)],
                                 flags=(3 * i + 8) % 16, soft=i % 4 == 2, seed=170 + i))
        for c in (1, 2, 3):
            out.append(_zoom("%s C=%d" % (fam, c), vols[c % 2], patch, _fit(r, DIMS, patch), triples[c], flags=c + 8, channels=c, soft=c == 2, seed=80 + c))
    return tuple(out)


def _affine(name, vol, patch, matrix, offset, flags=0, channels=4, soft=False, seed=0):
    v = volume(vol)
    gain, bias = _gain_bias(np.random.default_rng([SEED, 3, seed]), channels, v["exact"])
    m, o = np.array(matrix, np.float64).reshape(3, 3), np.array(offset, np.float64).reshape(3)
    _frozen(m, o)
    return dict(name="affine " + name, kind="affine", family="exact" if v["exact"] else "real", vol=vol, patch=tuple(patch), matrix=m, offset=o, flags=int(flags),
                C=channels, soft=bool(soft), gain=gain, bias=bias)


def rotation(angles):
    (c0, c1, c2), (s0, s1, s2) = np.cos(angles), np.sin(angles)
    r0 = np.array([[1.0, 0.0, 0.0], [0.0, c0, -s0], [0.0, s0, c0]])
    r1 = np.array([[c1, 0.0, s1], [0.0, 1.0, 0.0], [-s1, 0.0, c1]])
    r2 = np.array([[c2, -s2, 0.0], [s2, c2, 0.0], [0.0, 0.0, 1.0]])
    return r0 @ r1 @ r2 + 0.0


PERMS = (((0, 1, 2), (1, 1, 1)), ((1, 0, 2), (1, -1, 1)), ((2, 0, 1), (-1, 1, -1)), ((0, 2, 1), (-1, -1, 1)))


def _signed_perm(perm, signs, scales):
    m = np.zeros((3, 3))
    for row in range(3):
        m[row, perm[row]] = signs[row] * scales[row]
    return m


@functools.lru_cache(maxsize=None)
def affine_cases():
    r = np.random.default_rng([SEED, 4])
    out = []
    n = 0
    d, h, w = DIMS
    # exact: signed permutations times scales on the 0.25 grid, offsets on the 0.25 grid, crops that leave the volume on every side
    for si, patch in enumerate(SHAPES):
        for pi, (perm, signs) in enumerate(PERMS):
            scales = tuple(EXACT_SCALES[(si + pi + a) % 5] for a in range(3))                 # up to 2.5
            offset = [float(r.integers(-12, 4 * DIMS[a] - 4)) / 4.0 for a in range(3)]
            out.append(_affine("exact %s perm%d" % ("x".join(map(str, patch)), pi), ("exact", "exact_full")[n % 2], patch, _signed_perm(perm, signs, scales),
                               offset, flags=(7 * n + 2) % 16, channels=(4, 1, 2, 3)[n % 4] if si == 3 else 4, soft=n % 3 == 1, seed=n))
            n += 1
    # edge coordinates, exact family: the identity (and a unit flip) with offsets that put source coordinates exactly on -2, -1, -0.5, 0, n - 1, n - 0.5, n
    # and beyond both clamps
    eye = np.eye(3)
    edge = (("low", eye, (-3.0, -2.5, -3.0)), ("high", eye, (d - 3.0, h - 3.5, w - 5.0)), ("mixed", eye, (-2.5, h - 3.0, -1.0)),
            ("mirror", np.diag([-1.0, 1.0, -1.0]), (2.0, -3.0, w + 1.0)), ("half", eye * 0.5 + 0.0, (-2.0, h - 2.5, w - 3.0)))
    for ei, (tag, m, off) in enumerate(edge):
        for vi, vol in enumerate(("exact_full", "frac")):
            out.append(_affine("%s edge %s" % ("exact" if vi == 0 else "real", tag), vol, SHAPES[3], m, off, flags=(3 * ei + 8 * vi) % 16, soft=ei == 2, seed=30 + ei))
    # real: rotations about the patch centre, zoomed, and an explicit shear; crops across the tissue box and across the volume's faces
    angle_sets = ((np.pi / 6, 0.0, 0.0), (0.0, np.pi / 6, 0.0), (0.0, 0.0, np.pi / 6), (0.3, -0.2, 0.5), (np.pi / 2, 0.0, 0.0), (0.0, 0.0, 0.0))
    for si, patch in enumerate(SHAPES + (TIE_PATCH,)):
        for ai, angles in enumerate(angle_sets):
            if si < 3 and ai % 2:
                continue
            m = rotation(np.array(angles)) * np.array(REAL_SCALES[(si + ai) % 2])[None, :]
            half = (np.array(patch, np.float64) - 1.0) / 2.0
            lo = np.array([r.integers(-3, DIMS[a] - patch[a] + 4) for a in range(3)], np.float64)
            out.append(_affine("real %s rot%d" % ("x".join(map(str, patch)), ai), ("brats", "frac")[n % 2], patch, m, (lo + half) - m @ half,
                               flags=(7 * n + 2) % 16, channels=(4, 1, 2, 3)[n % 4] if si == 3 else 4, soft=n % 3 == 1, seed=n))
            n += 1
    shear = np.array([[0.9, 0.2, 0.0], [-0.1, 1.1, 0.3], [0.0, -0.2, 0.8]])
    for i in range(1, 9, 2):                                                                 # the affine half of the mixed launches
        perm, signs = PERMS[i % 4]
        out.append(dict(_affine("exact batch mixed %d" % i, ("exact", "exact_full")[(i // 2) % 2], BATCH_PATCH, _signed_perm(perm, signs, (0.75, 1.25, 2.5)),
                                (3.25, 9.5 - i, 14.75), flags=(5 * i) % 16, soft=i % 4 == 1, seed=180 + i), mapping=("row", "brick", "default")[(i // 2) % 3]))
        out.append(dict(_affine("real batch mixed %d" % i, ("brats", "frac")[(i // 2) % 2], BATCH_PATCH, shear * (1.0 + 0.05 * i), (3.5 + i, -1.25, 9.0 - i),
                                flags=(5 * i) % 16, soft=i % 4 == 1, seed=190 + i), mapping=("row", "brick", "default")[(i // 2) % 3]))
    for flags in range(16):
        perm, signs = PERMS[flags % 4]
        out.append(_affine("exact flags %d" % flags, ("exact", "exact_full")[flags % 2], SHAPES[3], _signed_perm(perm, signs, (1.25, 0.75, 2.5)),
                           (4.25, 11.5 - flags, 20.75), flags=flags, soft=flags % 4 == 2, seed=90 + flags))
    for flags in range(16):
        out.append(_affine("real flags %d" % flags, ("brats", "frac")[flags % 2], SHAPES[3], shear, (3.5, -1.25, 9.0), flags=flags, soft=flags % 4 == 1, seed=70 + flags))
    return tuple(out)


def _warp(name, patch, exact, disp, flags=0, channels=4, targets=3, seed=0):
    r = np.random.default_rng([SEED, 5, seed])
    patch = tuple(patch)
    if exact:
        data = r.integers(0, 4096, size=(channels,) + patch).astype(np.float32)
    else:
        data = (r.standard_normal((channels,) + patch) * 3.0).astype(np.float32)
    target = r.integers(0, 2, size=(targets,) + patch).astype(np.float32)
    if targets and not exact:
        target[0] = r.random(patch).astype(np.float32)                                      # order 0 copies any float, not only 0 / 1
    gain, bias = _gain_bias(r, channels, exact)
    disp = np.ascontiguousarray(disp, np.float64)
    _frozen(data, target, disp)
    return dict(name="warp " + name, kind="warp", family="exact" if exact else "real", patch=patch, data=data, target=target, disp=disp, flags=int(flags), C=channels,
                T=targets, gain=gain, bias=bias)


def _edge_disp(patch, r):
    """displacements whose coordinates land on k + 0.5 exactly, on negative fractions, beyond 2 n, and that are NaN, +-1e9 or +-inf"""
    disp = np.round(r.uniform(-2.0, 2.0, (3,) + patch) * 4.0) / 4.0
    flat = disp.reshape(3, -1)
    v = flat.shape[1]
    specials = (0.5, -0.5, 1.5, -1.5, 2.5, np.nan, 1.0e9, -1.0e9, np.inf, -np.inf, 2.0 * max(patch) + 0.75, -3.0 * max(patch) - 0.25, -0.25, 0.999999999)
    for i, s in enumerate(specials):
        flat[i % 3, (7 * i + 1) % v] = s
        flat[(i + 1) % 3, (11 * i + 3) % v] = s
    for ax in range(3):                                                                      # index 0 pushed to a negative fraction on every axis
        flat[ax, 0] = -0.75 - ax
    return disp


@functools.lru_cache(maxsize=None)
def warp_cases():
    r = np.random.default_rng([SEED, 6])
    out = []
    n = 0
    for si, patch in enumerate(SHAPES + (TIE_PATCH,)):
        for exact in (True, False):
            for kind in ("smooth", "far", "edge"):
                if kind == "edge":
                    disp = _edge_disp(patch, r)
                else:
                    amp = 2.0 if kind == "smooth" else 3.0 * max(patch)                      # far: beyond one reflection, the periodic part
                    disp = r.uniform(-amp, amp, (3,) + patch)
                    if exact:
                        disp = np.round(disp * 4.0) / 4.0
                if exact and kind == "edge":
                    disp = np.where(np.isfinite(disp), np.round(disp * 4.0) / 4.0, disp)
                out.append(_warp("%s %s %s" % ("exact" if exact else "real", "x".join(map(str, patch)), kind), patch, exact, disp, flags=(5 * n + 1) % 16,
                                 seed=n))
                n += 1
    patch = SHAPES[3]
    for flags in range(16):
        exact = flags % 2 == 0
        disp = r.uniform(-4.0, 4.0, (3,) + patch)
        out.append(_warp("%s flags %d" % ("exact" if exact else "real", flags), patch, exact, np.round(disp * 4.0) / 4.0 if exact else disp, flags=flags, seed=100 + flags))
    for c, t in ((0, 3), (2, 0), (1, 1), (3, 8), (8, 2)):                                    # a count of 0 skips that group and its pointers
        out.append(_warp("real C=%d T=%d" % (c, t), patch, False, r.uniform(-3.0, 3.0, (3,) + patch), flags=(c + t) % 16, channels=c, targets=t, seed=120 + c))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def two_pass_cases():
    """the three cases whose patch exceeds a grid cap (CAP_ZOOM for the zoom pass, the affine row mapping and a packed zoom-only launch; CAP_WARP for
    the warp), so that voxels are produced by a second grid-stride pass"""
    r = np.random.default_rng([SEED, 7])
    gain, bias = _gain_bias(r, 2, False)
    zoom = dict(name="zoom two-pass", kind="zoom", family="real", vol="big", patch=BIG_PATCH, lo=(3, 4, 2), scale=(0.9, 1.1, 1.2), flags=5, C=2, soft=False,
                gain=gain, bias=bias)
    m = rotation(np.array((0.3, -0.2, 0.5))) * np.array((0.9, 1.1, 1.2))[None, :]
    half = (np.array(BIG_PATCH, np.float64) - 1.0) / 2.0
    off = (np.array((2.0, 3.0, 1.0)) + half) - m @ half
    _frozen(m, off)
    affine = dict(name="affine two-pass", kind="affine", family="real", vol="big", patch=BIG_PATCH, matrix=m, offset=off, flags=6, C=2, soft=False, gain=gain,
                  bias=bias)
    warp = _warp("two-pass", WARP_BIG, False, r.uniform(-3.0, 3.0, (3,) + WARP_BIG), flags=3, channels=1, targets=1, seed=200)
    return zoom, affine, warp


def all_cases():
    return zoom_cases() + affine_cases() + warp_cases()


def by_name(name):
    for c in all_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- taps
def reflect(i, n):
    """half-sample symmetric extension (d c b a | a b c d | d c b a), periodic in 2 n"""
    i = np.mod(i, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def _reflect_mutant(i, n, mutant):
    if mutant == "whole_sample_reflect":                                                     # (d c b | a b c d | c b a), period 2 n - 2
        if n == 1:
            return np.zeros_like(i)
        i = np.mod(i, 2 * n - 2)
        return np.where(i < n, i, 2 * n - 2 - i)
    if mutant == "reflect_no_period":                                                        # one reflection, then the edge
        return np.clip(np.where(i < 0, -1 - i, np.where(i < n, i, 2 * n - 1 - i)), 0, n - 1)
    return reflect(i, n)


def zoom_weight(index, scale):
    """(i0 int64, t float32) for integer output indices: i0 = floor(fl64(index * scale)), t = float32(index * scale - i0) with the product exact"""
    idx = np.asarray(index, np.int64)
    f = np.floor(idx.astype(np.float64) * np.float64(scale))
    if np.finfo(np.longdouble).nmant >= 63:                                                  # < 11 + 53 bits: the product is exact in a 64-bit mantissa
        assert idx.size == 0 or int(np.abs(idx).max()) < 2048
        t = (idx.astype(np.longdouble) * np.longdouble(np.float64(scale)) - f.astype(np.longdouble)).astype(np.float32)
    else:
        from fractions import Fraction
        t = np.array([np.float32(float(Fraction(int(i)) * Fraction(float(scale)) - Fraction(float(g)))) for i, g in zip(idx.reshape(-1), f.reshape(-1))],
                     np.float32).reshape(idx.shape)
    return f.astype(np.int64), t


def _full(a, ax, patch):
    sh = [1, 1, 1]
    sh[ax] = patch[ax]
    return np.broadcast_to(np.asarray(a).reshape(sh), patch)


def zoom_taps(case, mutant=None):
    """per axis (i0, i1, in0, in1, t): cells as whole-volume indices, whether they are stored, the upper cell's float32 weight; arrays of the patch's shape"""
    taps = []
    patch = case["patch"]
    for ax in range(3):
        i0, t = zoom_weight(np.arange(patch[ax]), case["scale"][ax])
        lo = 0 if (mutant == "drop_crop_lo" and ax == 1) else case["lo"][ax]
        a, b = _reflect_mutant(i0, patch[ax], mutant) + lo, _reflect_mutant(i0 + 1, patch[ax], mutant) + lo
        ok = np.ones(patch[ax], bool)
        taps.append(tuple(_full(v, ax, patch) for v in (a, b, ok, ok, t)))
    return taps


def affine_taps(case, dims, mutant=None):
    patch, m, o = case["patch"], case["matrix"], case["offset"]
    q = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in patch], indexing="ij")
    taps = []
    for ax in range(3):
        s = ((m[ax, 0] * q[0] + m[ax, 1] * q[1]) + m[ax, 2] * q[2]) + o[ax]
        s = np.where(s >= -2.0, s, -2.0)
        s = np.minimum(s, float(dims[ax]))
        f = np.trunc(s) if mutant == "trunc_not_floor" else np.floor(s)
        i0 = f.astype(np.int64)
        t = (s - f).astype(np.float32)
        in0, in1 = (i0 >= 0) & (i0 < dims[ax]), (i0 + 1 >= 0) & (i0 + 1 < dims[ax])
        if mutant == "clamp_to_edge":
            in0 = in1 = np.ones(patch, bool)
        taps.append((np.clip(i0, 0, dims[ax] - 1), np.clip(i0 + 1, 0, dims[ax] - 1), in0, in1, t))
    return taps


def warp_taps(case, mutant=None):
    """the taps of the order-1 channels and `near`, the order-0 cell per axis"""
    patch, disp = case["patch"], case["disp"]
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in patch], indexing="ij")
    taps, near = [], []
    ok = np.ones(patch, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for ax in range(3):
            c = grid[ax] + disp[ax]
            c = np.where(np.abs(c) < 1.0e9, c, 0.0)                                          # NaN, +-inf and |c| >= 1e9 read as 0
            f = np.trunc(c) if mutant == "trunc_not_floor" else np.floor(c)
            i0 = f.astype(np.int64)
            t = (c - f).astype(np.float32)
            n = patch[ax]
            taps.append((_reflect_mutant(i0, n, mutant), _reflect_mutant(i0 + 1, n, mutant), ok, ok, t))
            pick = np.rint(c) if mutant == "round_half_even" else np.floor(c + 0.5)
            near.append(_reflect_mutant(pick.astype(np.int64), n, mutant))
    return taps, near


# ---------------------------------------------------------------------------------------------------------------- the eight corners
def _fma32(w, x, acc):
    return (w.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def corners(taps, chans, emu=False, fused=True, mutant=None, pre=None):
    """(acc, S, floor) [K, P0, P1, P2] of chans [K, D, H, W]: acc = sum_q w_q x_q over the eight corners, S = sum_q |w_q| |x_q| and the underflow
    floor TINY (sum_q |x_q| + 8), both float64 always.
    emu: the kernels' float32 order -- w = (wa * wb) * wc, then fmaf(w, x, acc) per corner (fused) or acc + w * x with both roundings.
    pre [K]: subtracted from every STORED corner value before the weighting (the mean_before_fill mutant)."""
    shape = taps[0][0].shape
    k = chans.shape[0]
    acc = np.zeros((k,) + shape, np.float32 if emu else np.float64)
    mag = np.zeros((k,) + shape, np.float64)
    xsum = np.zeros((k,) + shape, np.float64)
    wgt = []
    for ax in range(3):
        t = taps[ax][4]
        lo_w, hi_w = (np.float32(1.0) - t, t) if emu else (1.0 - t.astype(np.float64), t.astype(np.float64))
        if mutant == "swap_weights" and ax == 2:
            lo_w, hi_w = hi_w, lo_w
        wgt.append((lo_w, hi_w))
    for q in range(8):
        qs = (q >> 2, (q >> 1) & 1, q & 1)
        w = (wgt[0][qs[0]] * wgt[1][qs[1]]) * wgt[2][qs[2]]                                  # float32 arrays round after each product
        ok = taps[0][2 + qs[0]] & taps[1][2 + qs[1]] & taps[2][2 + qs[2]]
        x = chans[:, taps[0][qs[0]], taps[1][qs[1]], taps[2][qs[2]]]
        if pre is not None:
            x = x - np.asarray(pre, x.dtype).reshape(-1, 1, 1, 1)
        x = np.where(ok[None], x, 0)
        mag += np.abs(w.astype(np.float64))[None] * np.abs(x.astype(np.float64))
        xsum += np.abs(x.astype(np.float64))
        if not emu:
            acc += w[None] * x.astype(np.float64)
        elif fused:
            acc = _fma32(np.broadcast_to(w[None], x.shape), x.astype(np.float32), acc)
        else:
            acc = acc + w[None] * x.astype(np.float32)
    return acc, mag, TINY * (xsum + 8.0)


def finish(t, flags, mutant=None):
    """[K, P0, P1, P2] in source order -> the output layout [K, Q0, Q1, P2]: flips (bits 0..2), then the D <-> H transpose (bit 3)"""
    tr = bool(flags & 8)
    if mutant == "flip_after_transpose" and tr:
        t = t.transpose((0, 2, 1, 3))
        for ax in range(3):
            if flags & (1 << ax):
                t = np.flip(t, axis=ax + 1)
        return np.ascontiguousarray(t)
    for ax in range(3):
        if flags & (1 << ax):
            t = np.flip(t, axis=ax + 1)
    if tr and mutant == "swap_q":                                                            # the linear index decoded with the extents the wrong way round
        return np.ascontiguousarray(t).reshape(t.shape[0], t.shape[2], t.shape[1], t.shape[3])
    return np.ascontiguousarray(t.transpose((0, 2, 1, 3)) if tr else t)


def _repeat_pass(t, cap):
    """a second grid-stride pass that computes the first pass's voxels again: linear index o >= cap gets the value of o - cap"""
    if t is None:
        return None
    flat = t.reshape(t.shape[0], -1).copy()
    if flat.shape[1] > cap:
        flat[:, cap:] = flat[:, :flat.shape[1] - cap]
    return flat.reshape(t.shape)


def _sources(case, mutant):
    v = volume(case["vol"])
    c = case["C"]
    image, label, soft = v["image"][:c], v["label"], v["soft"]
    if mutant == "box_forgets_lo":                                                           # a packed source that reads box index idx instead of idx - lo, axis 2
        lo, size = v["box"][0][2], v["box"][1][2]

        def shift(a):
            out = np.zeros_like(a)
            out[..., :size] = a[..., lo:lo + size]
            return out
        image, label, soft = shift(image), shift(label), shift(soft)
    return v, image, label, soft


def run(case, mode="ref", mutant=None, cap=None, fused=True):
    """dict(data, target, bar_data, bar_target) of a case, arrays in the output layout.  mode "ref": float64, the definition; "emu": the kernel's float32
    operation order (`fused`: the warp loop's two allowed forms).  Bars are 0 in the exact family and for order-0 targets."""
    assert mode in ("ref", "emu") and (mutant is None or mutant in MUTANTS)
    emu = mode == "emu"
    flags, c = case["flags"], case["C"]
    gain, bias = case["gain"], case["bias"]
    if mutant == "neighbour_gain":
        gain = np.roll(gain, -1)
    if mutant == "neighbour_bias":
        bias = np.roll(bias, -1)
    sh = (-1, 1, 1, 1)
    exact = case["family"] == "exact"
    if case["kind"] == "warp":
        taps, near = warp_taps(case, mutant)
        out = dict(data=None, target=None, bar_data=None, bar_target=None)
        if c:
            acc, mag, floor = corners(taps, case["data"], emu, fused, mutant)
            if emu and fused:
                res = _fma32(acc, np.broadcast_to(gain.reshape(sh), acc.shape), np.broadcast_to(bias.reshape(sh), acc.shape))
            elif emu:
                res = acc * gain.reshape(sh) + bias.reshape(sh)
            else:
                res = acc * gain.astype(np.float64).reshape(sh) + bias.astype(np.float64).reshape(sh)
            g = np.abs(gain.astype(np.float64)).reshape(sh)
            bar = U * (12.0 * mag * g + np.abs(acc.astype(np.float64)) * g + np.abs(res.astype(np.float64))) + floor * g
            out["data"], out["bar_data"] = finish(res, flags, mutant), finish(bar * (0.0 if exact else 1.0), flags, mutant)
        if case["T"]:
            out["target"] = finish(case["target"][:, near[0], near[1], near[2]], flags, mutant)
            out["bar_target"] = np.zeros(out["target"].shape)
        if mutant == "second_pass_repeats":
            out["data"], out["target"] = _repeat_pass(out["data"], cap), _repeat_pass(out["target"], cap)
        return out
    v, image, label, soft = _sources(case, mutant)
    taps = zoom_taps(case, mutant) if case["kind"] == "zoom" else affine_taps(case, v["dims"], mutant)
    mean, istd = v["mean"][:c], v["istd"][:c]
    pre = mean if mutant == "mean_before_fill" else None
    acc, mag, floor = corners(taps, image, emu, True, mutant, pre)
    if emu:
        z = ((acc - (0 if pre is not None else mean.reshape(sh))) * istd.reshape(sh)).astype(np.float32)
        res = _fma32(z, np.broadcast_to(gain.reshape(sh), z.shape), np.broadcast_to(bias.reshape(sh), z.shape))
    else:
        m64 = 0.0 if pre is not None else mean.astype(np.float64).reshape(sh)
        res = ((acc - m64) * istd.astype(np.float64).reshape(sh)) * gain.astype(np.float64).reshape(sh) + bias.astype(np.float64).reshape(sh)
    ig = np.abs(istd.astype(np.float64) * gain.astype(np.float64)).reshape(sh)
    bar = U * ((11.0 * mag + 2.0 * (mag + np.abs(mean.astype(np.float64)).reshape(sh))) * ig + np.abs(res.astype(np.float64))) + floor * ig
    if case["soft"]:
        tgt, tmag, tfloor = corners(taps, soft, emu, True, mutant)
        tbar = U * 11.0 * tmag + tfloor
    else:
        onehot = np.stack([label == 1, label == 2, label == 3]).astype(np.float32)
        cw, wmag, wfloor = corners(taps, onehot, emu, True, mutant)
        tc = cw[0] + (cw[1] if mutant == "tc_1_plus_2" else cw[2])
        tgt = np.stack([(cw[0] + cw[1]) + cw[2], tc, cw[2]])
        tbar = U * np.stack([13.0 * (wmag[0] + wmag[1] + wmag[2]), 12.0 * (wmag[0] + wmag[2]), 11.0 * wmag[2]]) + wfloor.sum(axis=0)[None]
    zero = 0.0 if exact else 1.0
    out = dict(data=finish(res, flags, mutant), target=finish(tgt, flags, mutant), bar_data=finish(bar * zero, flags, mutant),
               bar_target=finish(tbar * zero, flags, mutant))
    if mutant == "second_pass_repeats":
        out["data"], out["target"] = _repeat_pass(out["data"], cap), _repeat_pass(out["target"], cap)
    return out


def worst_ratio(got, want, bar):
    """(max over voxels of |got - want| / bar, with 0 / 0 = 0 and x / 0 = inf; index of the worst voxel)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bar)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), np.unravel_index(i, ratio.shape)
