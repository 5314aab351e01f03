"""Seeded cases, the float64 restatement, per-voxel bars, a float32 emulation and mutants of the intensity augmentation (csrc/intensity.hip,
`ru_intensity_augment`), shared by tests/test_intensity_f64_host.py (no GPU) and tests/test_intensity_f64.py (the kernels).  Plain numpy.

WHAT THE RESTATEMENT DEFINES (`run(case)`, mode "ref").  Everything the kernels receive as float32 is float32 here too -- the 17 blur weights
(float32(e_d / sum e), e in float64, as the entry forms them), the low-res t = float32(rem / 2P), sd = float32(sqrt(variance)), brightness,
contrast factor, gamma, the constant float32(1e-7), and the statistics where `int_pointwise_kernel` loads them into `IntChan` (c_mean, c_min,
c_max, g_min, g_range, r_mean, r_mean_y, r_scale: each a cast of a float64 statistic) -- and everything after that is float64: the three blur
passes, the seven lerps, n = sqrt(-2 ln u1) cos(2 pi u2) on the exact 53-bit draws, the chain, 1 / (range + 1e-7), t^g, the statistics
themselves (numpy mean / std / min / max of the float64 channel as it enters the stage).  tests/test_intensity_f64_host.py ties it to
`dataloader.intensity_augment_host` and to scipy at a tolerance derived from those parameter roundings.  All inputs are finite; non-finite
input is out of scope (the kernels promise nothing for it, and `0 * inf` in a zero-weight tap is one reason).

THE BARS are per voxel.  A float32 rounding is allowed rnd(v) = 2^-24 |v| + 2^-149 of the value it forms (the second term: a result in the
subnormal range), a stage's input bar is carried through the stage's Lipschitz factor, and the count per stage is read off the kernel text:
  blur        per axis 2r + 1 fmaf (a zero weight adds +0 exactly), each on a partial sum |.| <= S = sum_k |w_k| |x_k|:
              bar_out = sum_k |w_k| bar_in_k + (2r + 1) rnd(S), three times.
  low-res     per lerp x0 + t (x1 - x0): the difference, the product (none if the compiler contracts it) and the sum:
              bar_out = (1 - t) bar_0 + t bar_1 + rnd(x1 - x0) t + rnd(t (x1 - x0)) + rnd(result); seven lerps, axis 2 first.
  noise       n: see NOISE below; x + sd n: sd bar_n + rnd(sd n) + rnd(sum).       brightness   |b| bar_in + rnd(x b).
  statistics  sums are float64: 64 roundings of 2^-53 on mean |x| (32 per thread, 6 butterfly, 3 waves, 1 + 8 final, the division, spare)
              = SUM64 mean|x| on the mean, the same on E[x^2] and mean^2 for the variance; the voxels' own bars move the mean by at most their
              mean, min / max by at most what the interval [x - bar, x + bar] allows, and std by at most their RMS (std is a seminorm).
              A float32 load of a statistic a known to e: e + 2 rnd(|a| + e).
  contrast    (x - m) f + m, clipped: |f| (bar_in + e_m + rnd(x - m)) + rnd((x - m) f) + e_m + rnd(result); the clip is 1-Lipschitz in value
              and bounds: max(that, e_min, e_max), and just that where the value stays clear of both bounds by the errors.
  gamma       d = x - min: bar_in + e_min + rnd(d); inv = 1 / (range + 1e-7): e_range + rnd(range + 1e-7) through inv^2, + rnd(inv);
              t = d inv: e_d inv + d e_inv + rnd(t), and a t below 2^-126 may count as 0 (v_log_f32 takes no denormals): e_t >= t there.
              t^g is monotone, so the input error is carried as max(|(t +- e_t)^g - t^g|) -- no derivative, t^g is not Lipschitz at 0 for g < 1;
              its own error is t^g ln2 (|g log2 t| (1 + ULP_LOG2) + ULP_EXP2) 2^-24 (log2 to ULP_LOG2, the product g L rounded, exp2 to
              ULP_EXP2) + 2^-126 (a subnormal result may be flushed); y = p range + min: e_p range + p e_range + rnd(p range) + e_min + rnd(y).
  retain      scale = std_x / max(std_y, 1e-8): e_sx / sy + sx e_sy / sy^2 (sy, sx at their unfavourable ends) + the float32 load;
              (y - my) scale + mx: (|scale| + e_scale)(bar_y + e_my + rnd(y - my)) + |y - my| e_scale + rnd(product) + e_mx + rnd(result).
              std_x / std_y is the amplification: a channel gamma flattens carries every earlier error times that ratio.
NOISE.  With h = float32(u1) the kernel takes ln u1 = L = logf(h) + float32(u1 - h) / h (the difference exact in float64; ln(1 + d) - d <= 2^-51):
logf to ULP_LOGF 2^-24 |ln h|, the cast and the division 2 rnd(d), the sum rnd(L); -2 L is exact and sqrtf correctly rounded, so R = sqrt(-2 L)
is good to R (e_L / 2L + 2^-25), and exactly 0 at u1 = 1.  The angle a = 2 pi u2 (reduced in float64) is rounded to float32: |a| 2^-24 |sin a| on
the cosine, which is itself good to ULP_COS 2^-24 |cos a| + 2^-149; the product rounds once.  The ULP_* constants are measured on an MI355X by
tools/libm_ulp.py on exactly the arguments these cases produce, rounded up, plus one (figures beside the constants).  `noise_u1_float32` (logf(h)
alone, the kernel's former behaviour: 3e-8 absolute on a logarithm of 1e-7, n = 0 for every u1 in (1 - 2^-25, 1]) is a mutant.

`run(case, "emu", mutant=None)` evaluates a case in the kernels' float32 operation order -- fmaf(w, x, acc) as float32(float64(w) float64(x) +
float64(acc)), chains in tap order, independent of the tiling, the float64 sums in the partial -> final order of `int_pointwise_kernel` /
`int_stats_final_kernel` on either route -- with numpy's float32 log2 / exp2 / log / cos standing in for the device's (the ULP
allowance covers the difference); `mutant` names one deliberate defect of MUTANTS, each with the case that shows it."""
import functools
import math

import numpy as np

SEED = 20197
U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MIN = 2.0 ** -126
SUM64 = 64 * 2.0 ** -53
EPS7 = float(np.float32(1e-7))
CHUNK = 8192
M64 = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

# measured on an MI355X by tools/libm_ulp.py on the arguments of these cases, in units of 2^-24 |y|; the bar carries ceil(measured) + 1
# v_log_f32 (__builtin_amdgcn_logf) 1.9736, v_exp_f32 (__builtin_amdgcn_exp2f) 1.4140, logf 3.0298, cosf 2.0230
MEASURED = {"log2": 1.9736, "exp2": 1.4140, "logf": 3.0298, "cosf": 2.0230}
ULP_LOG2, ULP_EXP2, ULP_LOGF, ULP_COS = (float(math.ceil(MEASURED[k]) + 1) for k in ("log2", "exp2", "logf", "cosf"))
assert math.log(2.0) * ULP_EXP2 >= MEASURED["exp2"]           # gamma's term holds ULP_EXP2 under the factor ln2: still above what v_exp_f32 was measured at

STAGES = ("blur", "lowres", "noise", "brightness", "contrast", "gamma", "retain")
FAMILIES = ("unit", "brats", "raw", "offset", "constant", "two", "negative", "tiny")
GRID_SHAPES = ((1, 1, 1), (1, 1, 4), (5, 6, 7), (17, 3, 8), (3, 34, 132), (2, 33, 131), (8, 16, 64), (3, 3, 911))
GAMMAS, CONTRASTS, SIGMAS, ZOOMS = (0.25, 0.7, 1.0, 1.5, 4.0), (0.75, 1.0, 1.25), (0.5, 0.62, 1.0, 2.0), (0.05, 0.5, 0.63, 1.0)
NOISE_SEEDS = (1, 7, (1 << 63) + 12345, (1 << 64) - 5)


# what a rounding is worth.  "device": the bars -- every arithmetic rounding 2^-24, a parameter's own rounding nothing (both sides hold the float32 parameter).
# "host": the tolerance between this restatement and a pure float64 one (dataloader.intensity_augment_host, scipy) -- every arithmetic rounding 2^-52 (two
# float64 sides), every parameter the restatement holds in float32 one 2^-24 of the product it enters (`prm`), no flush of subnormals.
_MODEL = {"u": U, "prm": 0.0, "device": True}


def rnd(v):
    return _MODEL["u"] * np.abs(v) + TINY


def prm(v):
    return _MODEL["prm"] * np.abs(v)


# ---------------------------------------------------------------------------------------------------------------- the generator and its inverse
def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * MIX1) & M64
    z = ((z ^ (z >> 27)) * MIX2) & M64
    return z ^ (z >> 31)


def unmix64(y):
    """mix64 is a bijection of 64-bit words: each xor-shift and each odd multiply is invertible mod 2^64"""
    y &= M64
    y = y ^ (y >> 31) ^ (y >> 62)
    y = (y * pow(MIX2, -1, 1 << 64)) & M64
    y = y ^ (y >> 27) ^ (y >> 54)
    y = (y * pow(MIX1, -1, 1 << 64)) & M64
    return y ^ (y >> 30) ^ (y >> 60)


def _mix64_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
    return z ^ (z >> np.uint64(31))


def draws(seed, channel, count, mutant=None):
    """(u1, u2) of voxels 0 .. count-1, float64, exact: u1 = ((z1 >> 11) + 1) 2^-53 in (0, 1], u2 = (z2 >> 11) 2^-53 in [0, 1)"""
    key = mix64(int(seed) + (1 if mutant == "noise_key_ignores_channel" else channel + 1) * GOLDEN)
    v = np.arange(int(count), dtype=np.uint64) + np.uint64(1 if mutant == "noise_voxel_plus_1" else 0)
    with np.errstate(over="ignore"):
        z1 = _mix64_np(np.uint64(key) + (np.uint64(2) * v + np.uint64(1)) * np.uint64(GOLDEN))
        z2 = _mix64_np(np.uint64(key) + (np.uint64(2) * v + np.uint64(2)) * np.uint64(GOLDEN))
    if mutant == "noise_swap_z":
        z1, z2 = z2, z1
    return ((z1 >> np.uint64(11)).astype(np.float64) + 1.0) / 2.0 ** 53, (z2 >> np.uint64(11)).astype(np.float64) / 2.0 ** 53


def seed_for(channel, which, bits53, low11=0):
    """the seed whose voxel 0 of `channel` draws z1 (which = 1) or z2 (which = 2) = bits53 << 11 | low11"""
    key = (unmix64((bits53 << 11) | low11) - which * GOLDEN) & M64
    return (unmix64(key) - (channel + 1) * GOLDEN) & M64


# name -> (which draw, its 53 bits, the u it gives): u1 = (bits + 1) 2^-53, u2 = bits 2^-53
NOISE_EDGES = {
    "u1 = 1 - 2^-30": (1, (1 << 53) - (1 << 23) - 1, 1.0 - 2.0 ** -30),          # float32(u1) = 1: the former kernel gave n = 0
    "u1 = 1 - 2^-24": (1, (1 << 53) - (1 << 29) - 1, 1.0 - 2.0 ** -24),
    "u1 = 2^-53": (1, 0, 2.0 ** -53),                                              # the largest radius, sqrt(106 ln 2) = 8.57
    "u2 = 0.5": (2, 1 << 52, 0.5),                                                 # the first angle that is reduced: -pi
    "u2 = 0.5 - 2^-53": (2, (1 << 52) - 1, 0.5 - 2.0 ** -53),                      # the last that is not: float32(pi)
    "u2 = 0.25": (2, 1 << 51, 0.25),                                               # cos = 0 but for the rounding of pi / 2
}


def edge_seed(name, channel):
    """a seed for NOISE_EDGES[name] at voxel 0 of `channel`; for the u1 edges the free low bits are walked until |cos| of the same voxel > 0.5"""
    which, bits, _ = NOISE_EDGES[name]
    for low in range(2048):
        seed = seed_for(channel, which, bits, low)
        if which == 2 or abs(math.cos(2.0 * math.pi * draws(seed, channel, 1)[1][0])) > 0.5:
            return seed
    raise AssertionError(name)


# ---------------------------------------------------------------------------------------------------------------- inputs and cases
def make_input(family, channels, shape, seed):
    """[channels, *shape] float32, finite, no -0"""
    r = np.random.default_rng([SEED, seed])
    full = (channels,) + tuple(shape)
    if family == "unit":
        x = r.standard_normal(full)
    elif family == "brats":                                    # exact 0 around a z-scored interior
        x = np.zeros(full)
        box = tuple(slice(n // 4, max(n - n // 4, n // 4 + 1)) for n in shape)
        inner = x[(slice(None),) + box]
        inner[...] = r.standard_normal(inner.shape)
        inner -= inner.mean(axis=(1, 2, 3), keepdims=True)
    elif family == "raw":
        x = r.integers(0, 65536, full).astype(np.float64)
    elif family == "offset":
        x = 1e4 + r.uniform(-1.0, 1.0, full)
    elif family == "constant":
        x = np.empty(full)
        for c in range(channels):
            x[c] = (0.3, 1e4, -2.5, 0.0, 65535.0, 1e-30, -1e4, 0.1)[c % 8]
    elif family == "two":
        x = np.where(r.random(full) < 0.3, 2.25, -1.5)
    elif family == "negative":
        x = -np.abs(r.standard_normal(full)) - 0.5
    elif family == "tiny":                                     # even channels: 1e-30 throughout (products underflow); odd: 0, subnormals and O(1), so that t is subnormal
        x = r.standard_normal(full) * 1e-30
        pick = r.random(full)
        odd = np.where(pick < 0.4, 0.0, np.where(pick < 0.7, r.uniform(1e-42, 1e-39, full), r.uniform(0.1, 1.0, full)))
        x[1::2] = odd[1::2]
    else:
        raise KeyError(family)
    x = x.astype(np.float32) + np.float32(0.0)                 # (-0 + 0 = +0)
    assert np.isfinite(x).all() and not np.signbit(x[x == 0]).any()
    x.setflags(write=False)
    return x


class _Cycle:
    def __init__(self, values, start=0):
        self.values, self.k = tuple(values), start

    def __call__(self):
        self.k += 1
        return self.values[(self.k - 1) % len(self.values)]


def _gamma_cycle():
    combos = [dict(gamma=g, gamma_invert=bool(k & 1), gamma_retain_stats=bool(k & 2)) for k in range(4) for g in GAMMAS]
    return _Cycle([combos[(3 * i) % 20] for i in range(20)])   # the 20 combinations, in steps of 3


def _mixes():
    """per-channel stage sets, drawn from cycles over every listed parameter value.  Of the first four every launch sees one that leaves at once and
    one that works: empty, blur only, blur + later stages, low-res + gamma without contrast (first = 1); then noise + contrast (kept at level
    0), brightness only (first = 3), all stages, gamma alone."""
    gam, con, sig, zoom, seed = _gamma_cycle(), _Cycle(CONTRASTS), _Cycle(SIGMAS), _Cycle(ZOOMS, 1), _Cycle(NOISE_SEEDS)
    var, bri = _Cycle((0.1, 0.02, 0.0)), _Cycle((1.25, 0.8, 1.0))
    kinds = (lambda: {},
             lambda: dict(blur_sigma=sig()),
             lambda: dict(blur_sigma=sig(), contrast=con(), **gam()),
             lambda: dict(lowres_zoom=zoom(), **gam()),
             lambda: dict(noise_variance=var(), noise_seed=seed(), contrast=con()),
             lambda: dict(brightness=bri()),
             lambda: dict(blur_sigma=sig(), lowres_zoom=zoom(), noise_variance=var(), noise_seed=seed(), brightness=bri(), contrast=con(), **gam()),
             lambda: gam())
    return kinds


def _case(name, shape, params, family, seed, in_off=0, out_off=0):
    return dict(name=name, shape=tuple(shape), C=len(params), params=params, family=family, seed=seed, in_off=in_off, out_off=out_off)


ALL_STAGES = dict(blur_sigma=1.0, lowres_zoom=0.63, noise_variance=0.1, noise_seed=4, brightness=1.25, contrast=0.75, gamma=1.5, gamma_invert=True, gamma_retain_stats=True)
TILE_MIX = [{}, dict(blur_sigma=2.0), dict(blur_sigma=1.0, contrast=1.25, gamma=1.5), dict(lowres_zoom=0.5, gamma=0.7, gamma_invert=True)]
REST = [{}, dict(blur_sigma=0.5), dict(lowres_zoom=0.5), dict(contrast=1.25)]     # fills a four-channel mix up to eight: one channel that leaves every launch but the write, one that leaves the write
ALIGN_MIX = [dict(blur_sigma=0.62), dict(ALL_STAGES), dict(noise_variance=0.1, noise_seed=7, contrast=1.25), dict(gamma=0.7, gamma_retain_stats=True)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    kinds = _mixes()
    k = 0
    for ci, channels in enumerate((1, 4, 8)):                  # every (family, C) pair once; every shape with every C
        for si, shape in enumerate(GRID_SHAPES):
            family = FAMILIES[(si + ci) % len(FAMILIES)]
            if channels == 1:
                params = [kinds[(2, 3, 4, 6, 7, 5, 1, 6)[si]]()]
            else:
                params = [kinds[(c + (si if channels == 4 else 0)) % 8]() for c in range(channels)]
                if not any(set(q) == {"blur_sigma"} for q in params):          # the channel that leaves the statistics launches and the write at once
                    params[si % 4] = kinds[1]()
                if not any(q == {} for q in params):
                    params[(si + 1) % 4] = {}
            out.append(_case("grid %s C%d %s" % ("x".join(map(str, shape)), channels, family), shape, params, family, k))
            k += 1
    # the tiles of int_blur_hw_kernel: two rows and two columns; 16-byte route with a 4-wide last column, scalar route with a 3-wide one
    out.append(_case("tiles float4", (3, 34, 132), TILE_MIX, "unit", 100))
    out.append(_case("tiles scalar", (2, 33, 131), TILE_MIX, "brats", 101))
    # the low-res load on its own, behind a blur (read from the second blur buffer) and in front of the noise, on both routes and across the 16-output column block
    lowres = [dict(lowres_zoom=0.5), dict(lowres_zoom=0.63), dict(blur_sigma=0.62, lowres_zoom=0.63), dict(blur_sigma=1.0), dict(lowres_zoom=0.63, noise_variance=0.02, noise_seed=7), dict(lowres_zoom=0.05),
              dict(blur_sigma=2.0, lowres_zoom=0.5, brightness=0.8), dict(lowres_zoom=0.5, contrast=1.25)]
    out.append(_case("lowres float4", (3, 34, 132), lowres, "unit", 105))
    out.append(_case("lowres scalar", (17, 3, 7), lowres[:4], "raw", 106))
    out.append(_case("ragged chunk", (3, 3, 911), [dict(noise_variance=0.02, noise_seed=1, contrast=1.25), dict(blur_sigma=0.5), dict(ALL_STAGES), {}], "unit", 102))
    # the same data on the 16-byte route and on the scalar route that a pointer one float past a 16-byte boundary forces (P2 % 4 == 0)
    out.append(_case("align base", (16, 40, 24), ALIGN_MIX, "unit", 103))
    out.append(_case("align in+1", (16, 40, 24), ALIGN_MIX, "unit", 103, in_off=1))
    out.append(_case("align out+1", (16, 40, 24), ALIGN_MIX, "unit", 103, out_off=1))
    # 260 partials: the second round of int_stats_final_kernel's strided loop.  No blur, no noise: the float64 side is a few reductions
    out.append(_case("260 partials", (130, 128, 128), [dict(contrast=1.25, gamma=0.7, gamma_retain_stats=True)], "unit", 104))
    for i, name in enumerate(NOISE_EDGES):                     # the constructed draws at voxel 0 of channel i % 4, one with contrast behind it
        c = i % 4
        q = dict(noise_variance=0.1, noise_seed=edge_seed(name, c))
        if i % 2:
            q["contrast"] = 1.25
        out.append(_case("noise " + name, (5, 6, 7), [q if j == c else ({} if j % 2 else dict(blur_sigma=0.5)) for j in range(4)], "unit", 110 + i))
    out.append(_case("offset retain", (5, 6, 7), [dict(gamma=1.5, gamma_retain_stats=True), dict(contrast=1.25, gamma=0.7, gamma_invert=True, gamma_retain_stats=True), dict(blur_sigma=1.0),
                                                  dict(blur_sigma=0.5, contrast=0.75)], "offset", 120))
    out.append(_case("constant gamma", (5, 6, 7), [dict(gamma=0.7), dict(gamma=1.5, gamma_retain_stats=True), dict(contrast=1.25, gamma=0.25, gamma_invert=True, gamma_retain_stats=True),
                                                   dict(blur_sigma=1.0, lowres_zoom=0.5, brightness=1.25, contrast=0.75, gamma=4.0, gamma_retain_stats=True)] + REST, "constant", 121))
    out.append(_case("order", (5, 6, 7), [dict(noise_variance=0.1, noise_seed=3, brightness=1.25), dict(brightness=1.25, contrast=0.75), dict(gamma=1.5, gamma_invert=True),
                                          dict(gamma=0.7, gamma_invert=True, gamma_retain_stats=True)] + REST, "unit", 122))
    out.append(_case("identities", (5, 6, 7), [dict(noise_variance=0.0, noise_seed=9), dict(lowres_zoom=1.0), dict(lowres_zoom=0.05), dict(brightness=1.25)] + REST, "unit", 123))
    out.append(_case("contrast clip", (5, 6, 7), [dict(contrast=1.25), {}, dict(contrast=0.75), dict(contrast=1.0)] + REST, "unit", 124))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    for c in cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def input_of(name):
    c = by_name(name)
    return make_input(c["family"], c["C"], c["shape"], c["seed"])


LAUNCHES = ("blur", "table", 0, 1, 2, 3)


def takes_part(q, launch):
    """whether a channel with parameters q works in a launch: the two blur kernels, the low-res table kernel, int_pointwise_kernel at level 0 (contrast
    statistics), 1 (gamma), 2 (retain-stats) and 3 (the write, which a blur-only channel leaves: the tile pass wrote it)"""
    if launch == "blur":
        return "blur_sigma" in q
    if launch == "table":
        return "lowres_zoom" in q
    return ("contrast" in q, "gamma" in q, bool(q.get("gamma_retain_stats")), set(q) != {"blur_sigma"})[launch]


def last_stage(q):
    """the stage a channel's output leaves: the key of the per-stage report"""
    for stage, key in (("retain", "gamma_retain_stats"), ("gamma", "gamma"), ("contrast", "contrast"), ("brightness", "brightness"), ("noise", "noise_variance"),
                       ("lowres", "lowres_zoom"), ("blur", "blur_sigma")):
        if q.get(key):
            return stage
    return "copy"


# ---------------------------------------------------------------------------------------------------------------- parameters as the entry forms them
def radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def blur_weights(sigma, mutant=None):
    """the 17 float32 taps: float32(e_d / sum e) for |d| <= r, 0 beyond"""
    sigma = float(sigma)
    r = radius(sigma) - (1 if mutant == "blur_radius_minus_1" else 0)
    e = [math.exp(-0.5 / (sigma * sigma) * float(d * d)) for d in range(-r, r + 1)]
    total = 0.0
    for v in e:
        total += v
    if mutant == "blur_unnormalised":
        total = 1.0
    w = np.zeros(17, np.float32)
    w[8 - r:8 + r + 1] = np.array([v / total for v in e], np.float64).astype(np.float32)
    return w, r


def reflect(i, n, mutant=None):
    """half-sample symmetric (d c b a | a b c d | d c b a), periodic in 2 n"""
    i = np.asarray(i, np.int64)
    if mutant == "blur_whole_sample_reflect":                  # (d c b | a b c d | c b a)
        if n == 1:
            return np.zeros_like(i)
        m = np.mod(i, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def lowres_axis(n, zoom, mutant=None):
    """(s0, s1, t float32) of one axis, in the kernel's integers"""
    n = int(n)
    nc = max(1, int(math.floor(n * float(zoom) + 0.5)))
    i = np.arange(n, dtype=np.int64)
    num = (2 * i + 1) * nc - n
    pos = num > 0
    j0 = np.where(pos, num // (2 * n), 0)
    rem = np.where(pos, num % (2 * n), 0)
    top = j0 >= nc - 1
    j0, rem = np.where(top, nc - 1, j0), np.where(top, 0, rem)
    j1 = np.minimum(j0 + 1, nc - 1)
    if mutant == "lowres_round_src":
        src = lambda j: np.minimum(((2 * j + 1) * n + nc) // (2 * nc), n - 1)
    else:
        src = lambda j: np.minimum(((2 * j + 1) * n) // (2 * nc), n - 1)
    return src(j0), src(j1), (rem.astype(np.float64) / float(2 * n)).astype(np.float32), nc


def f32(v):
    return np.float32(v)


def _bshape(ndim, ax):
    s = [1] * ndim
    s[ax] = -1
    return s


# ---------------------------------------------------------------------------------------------------------------- the restatement, with bars
def _stat_ref(x, bar):
    """float64 statistics of the channel and how far the device's (of values within `bar` of x, summed in float64) may lie from them"""
    ax = np.abs(x)
    mean, std, mn, mx = float(x.mean()), float(x.std()), float(x.min()), float(x.max())
    e_mean = float(bar.mean()) + SUM64 * float(ax.mean())
    e_min = max(mn - float((x - bar).min()), float((x + bar).min()) - mn)
    e_max = max(float((x + bar).max()) - mx, mx - float((x - bar).max()))
    dv = 2.0 * SUM64 * float(((ax + bar) ** 2).mean())           # E[x^2] and mean^2, each to SUM64 of itself, before they cancel
    e_std = float(np.sqrt((bar ** 2).mean())) + max(math.sqrt(std * std + dv) - std, std - math.sqrt(max(std * std - dv, 0.0)))
    return dict(mean=mean, std=std, min=mn, max=mx, e_mean=e_mean, e_std=e_std, e_min=e_min, e_max=e_max)


def _load(a, e):
    """a statistic known to e, cast to float32 on both sides (against a float64 side: on this one only): (the float32 value as float64, its error)"""
    return float(np.float32(a)), e + 2.0 * float(rnd(abs(a) + e)) + float(prm(abs(a) + e))


def noise_ref(seed, channel, count):
    """(n float64, bar_n) per voxel"""
    u1, u2 = draws(seed, channel, count)
    L = -np.log(u1)
    R = np.sqrt(2.0 * L)
    h = u1.astype(np.float32).astype(np.float64)
    u = _MODEL["u"]
    e_L = ULP_LOGF * u * np.abs(np.log(h)) + 2.0 * rnd((u1 - h) / h) + rnd(L) + 2.0 ** -51
    a = np.where(u2 >= 0.5, u2 - 1.0, u2) * (2.0 * np.pi)
    c = np.cos(a)
    e_R = np.where(L > 0.0, R * (0.5 * e_L / np.where(L > 0.0, L, 1.0) + 0.5 * u), 0.0) + TINY
    amag = np.abs(a) if _MODEL["device"] else 2.0 * np.pi       # (the float64 sides round the unreduced angle)
    e_c = u * amag * np.abs(np.sin(a)) + ULP_COS * u * np.abs(c) + TINY
    return R * c, e_R * (np.abs(c) + e_c) + R * e_c + rnd(R * c)


def ref_channel(x32, q, channel, against="device"):
    """one channel: (float64 output, per-voxel bar); against="host": the tolerance against a float64 restatement with float64 parameters instead"""
    _MODEL.update(dict(u=U, prm=0.0, device=True) if against == "device" else dict(u=2.0 ** -52, prm=U, device=False))
    try:
        return _ref_channel(x32, q, channel)
    finally:
        _MODEL.update(u=U, prm=0.0, device=True)


def _ref_channel(x32, q, channel):
    x = x32.astype(np.float64)
    bar = np.zeros_like(x)
    if "blur_sigma" in q:
        w, r = blur_weights(q["blur_sigma"])
        w = w.astype(np.float64)
        for ax in range(3):
            n = x.shape[ax]
            idx = reflect(np.arange(-8, n + 8), n)
            xp, bp = np.take(x, idx, axis=ax), np.take(bar, idx, axis=ax)
            taps = [k for k in range(17) if w[k] != 0.0]
            win = lambda a, k: np.take(a, np.arange(k, k + n), axis=ax)
            x = sum(w[k] * win(xp, k) for k in taps)
            S = sum(abs(w[k]) * (np.abs(win(xp, k)) + win(bp, k)) for k in taps)
            bar = sum(abs(w[k]) * win(bp, k) for k in taps) + len(taps) * rnd(S) + prm(S)
    if "lowres_zoom" in q:
        for ax in (2, 1, 0):
            s0, s1, t, _ = lowres_axis(x.shape[ax], q["lowres_zoom"])
            t = t.astype(np.float64).reshape(_bshape(3, ax))
            x0, x1, b0, b1 = np.take(x, s0, axis=ax), np.take(x, s1, axis=ax), np.take(bar, s0, axis=ax), np.take(bar, s1, axis=ax)
            d = x1 - x0
            x = x0 + t * d
            bar = (1.0 - t) * b0 + t * b1 + t * rnd(np.abs(d) + b0 + b1) + rnd(t * (np.abs(d) + b0 + b1)) + rnd(np.abs(x) + b0 + b1) + prm(t * (np.abs(d) + b0 + b1))
            bar = np.where(t == 0.0, b0, bar)                  # x0 + 0 * (x1 - x0) = x0: exact, contracted or not
    if "noise_variance" in q:
        sd = float(f32(math.sqrt(float(q["noise_variance"]))))
        n, e_n = noise_ref(q["noise_seed"], channel, x.size)
        n, e_n = n.reshape(x.shape), e_n.reshape(x.shape)
        p = sd * n
        y = x + p
        bar = (bar + sd * e_n + prm(p) + rnd(np.abs(p) + sd * e_n) + rnd(np.abs(y) + bar + sd * e_n)) if sd != 0.0 else bar
        x = y
    if "brightness" in q:
        b = float(f32(q["brightness"]))
        x, bar = x * b, abs(b) * bar + rnd(np.abs(x * b) + abs(b) * bar) + prm(x * b)
    if "contrast" in q:
        f = float(f32(q["contrast"]))
        s = _stat_ref(x, bar)
        m, e_m = _load(s["mean"], s["e_mean"])
        lo, e_lo = _load(s["min"], s["e_min"])
        hi, e_hi = _load(s["max"], s["e_max"])
        d = x - m
        e_d = bar + e_m + rnd(np.abs(d) + bar + e_m)
        p = d * f
        e_p = abs(f) * e_d + rnd(np.abs(p) + abs(f) * e_d) + prm(p)
        y = p + m
        e_y = e_p + e_m + rnd(np.abs(y) + e_p + e_m)
        inside = (y - e_y > lo + e_lo) & (y + e_y < hi - e_hi)  # unclipped on both sides: the bounds' errors do not enter
        x, bar = np.clip(y, lo, hi), np.where(inside, e_y, np.maximum(e_y, max(e_lo, e_hi)))
    if "gamma" in q:
        g = float(f32(q["gamma"]))
        inv, retain = bool(q.get("gamma_invert")), bool(q.get("gamma_retain_stats"))
        if inv:
            x = -x
        s = _stat_ref(x, bar)
        mn, e_mn = _load(s["min"], s["e_min"])
        rng, e_rng = _load(s["max"] - s["min"], s["e_min"] + s["e_max"])
        r_mean, e_rmean = _load(s["mean"], s["e_mean"])
        den = rng + EPS7
        e_den = e_rng + float(rnd(den + e_rng)) + (0.0 if _MODEL["device"] else abs(EPS7 - 1e-7))
        iv = 1.0 / den
        e_iv = e_den / (den * max(den - e_den, TINY)) + float(rnd(iv))
        d = x - mn
        e_d = bar + e_mn + rnd(np.abs(d) + bar + e_mn)
        t = np.maximum(d * iv, 0.0)
        e_t = e_d * (iv + e_iv) + np.abs(d) * e_iv
        e_t = e_t + rnd(t + e_t)
        if _MODEL["device"]:
            e_t = np.where(t - e_t < FLT_MIN, np.maximum(e_t, t), e_t)                 # a subnormal t may count as 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            p = np.power(t, g)
            up, down = np.power(t + e_t, g) - p, p - np.power(np.maximum(t - e_t, 0.0), g)
            l2 = np.where(t > 0.0, np.abs(g * np.log2(np.where(t > 0.0, t, 1.0))), 0.0)
        p_hi = p + np.maximum(up, down)
        e_p = np.maximum(up, down) + p_hi * math.log(2.0) * (l2 * (1.0 + ULP_LOG2) + ULP_EXP2) * _MODEL["u"] + prm(p_hi * math.log(2.0) * l2) + (FLT_MIN if _MODEL["device"] else 0.0)
        pr = p * rng
        e_pr = e_p * (rng + e_rng) + p * e_rng
        e_pr = e_pr + rnd(np.abs(pr) + e_pr)
        y = pr + mn
        e_y = e_pr + e_mn
        e_y = e_y + rnd(np.abs(y) + e_y)
        if retain:
            sy = _stat_ref(y, e_y)
            my, e_my = _load(sy["mean"], sy["e_mean"])
            den_y, lo_y = max(sy["std"], 1e-8), max(sy["std"] - sy["e_std"], 1e-8)
            scale64 = s["std"] / den_y
            e_sc = s["e_std"] / lo_y + (s["std"] + s["e_std"]) * sy["e_std"] / (lo_y * den_y)
            scale, e_sc = _load(scale64, e_sc)
            d = y - my
            e_d = e_y + e_my + rnd(np.abs(d) + e_y + e_my)
            p = d * scale
            e_p = (abs(scale) + e_sc) * e_d + np.abs(d) * e_sc
            e_p = e_p + rnd(np.abs(p) + e_p)
            y = p + r_mean
            e_y = e_p + e_rmean
            e_y = e_y + rnd(np.abs(y) + e_y)
        x, bar = (-y if inv else y), e_y
    return x, bar


# ---------------------------------------------------------------------------------------------------------------- the emulation
def _fma32(w, x, acc):
    return (np.asarray(w, np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def stats_emu(x, vec, mutant=None):
    """(mean, std, min, max) float64 of a float32 channel in the kernels' order: per workgroup of 8192 voxels a thread's 32 values in its loop's
    order (16-byte route: 8 float4 1024 apart; scalar: 32 values 256 apart), xor butterflies over 64 lanes, ((w0 + w1) + w2) + w3; then thread t takes
    partials t, t + 256, .. and a tree 128, 64, .. 1 sums the threads.  Missing voxels add +0.0, which changes no float64 sum."""
    flat = np.asarray(x, np.float32).reshape(-1)
    V = flat.size
    nblk = -(-V // CHUNK)
    a = np.zeros(nblk * CHUNK, np.float64)
    a[:V] = flat
    lo, hi = np.full(nblk * CHUNK, np.inf), np.full(nblk * CHUNK, -np.inf)
    lo[:V], hi[:V] = flat, flat
    if vec:
        order = lambda b: b.reshape(nblk, 8, 256, 4).transpose(0, 2, 1, 3).reshape(nblk, 256, 32)
    else:
        order = lambda b: b.reshape(nblk, 32, 256).transpose(0, 2, 1)
    a = order(a)
    s1, s2 = np.zeros((nblk, 256)), np.zeros((nblk, 256))
    for j in range(32):
        s1 = s1 + a[:, :, j]
        s2 = s2 + a[:, :, j] * a[:, :, j]
    lane = np.arange(64)
    parts = []
    for s in (s1, s2):
        s = s.reshape(nblk, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ o]
        parts.append(((s[:, 0, 0] + s[:, 1, 0]) + s[:, 2, 0]) + s[:, 3, 0])
    pmin, pmax = lo.reshape(nblk, CHUNK).min(axis=1), hi.reshape(nblk, CHUNK).max(axis=1)
    if mutant == "stats_drop_last_partial_chunk" and V % CHUNK:
        parts, pmin, pmax = [p[:-1] for p in parts], pmin[:-1], pmax[:-1]
    if mutant == "stats_drop_partials_ge_256":
        parts, pmin, pmax = [p[:256] for p in parts], pmin[:256], pmax[:256]
    tot = []
    for p in parts:
        rounds = -(-max(p.size, 1) // 256)
        b = np.zeros(rounds * 256)
        b[:p.size] = p
        b = b.reshape(rounds, 256)
        r = np.zeros(256)
        for i in range(rounds):
            r = r + b[i]
        o = 128
        while o:
            r[:o] = r[:o] + r[o:2 * o]
            o >>= 1
        tot.append(r[0])
    mean = tot[0] / float(V)
    var = tot[1] / float(V - 1 if mutant == "stats_sample_variance" else V) - mean * mean
    return mean, math.sqrt(var) if var > 0.0 else 0.0, float(pmin.min()) if pmin.size else np.inf, float(pmax.max()) if pmax.size else -np.inf


def noise_emu(seed, channel, count, mutant=None, tap=None):
    u1, u2 = draws(seed, channel, count, mutant)
    if tap is not None:                                        # the arguments of logf and cosf, for tools/libm_ulp.py
        tap["log"].append(u1.astype(np.float32))
        tap["cos"].append((np.where(u2 >= 0.5, u2 - 1.0, u2) * 6.283185307179586476925).astype(np.float32))
    with np.errstate(divide="ignore"):
        if mutant == "noise_u1_float32":
            ln1 = np.log(u1.astype(np.float32))
        else:
            h = u1.astype(np.float32)
            ln1 = (np.log(h) + ((u1 - h.astype(np.float64)).astype(np.float32) / h).astype(np.float32)).astype(np.float32)
    ang = (np.where(u2 >= 0.5, u2 - 1.0, u2) * 6.283185307179586476925).astype(np.float32)
    return (np.sqrt(f32(-2.0) * ln1).astype(np.float32) * np.cos(ang).astype(np.float32)).astype(np.float32)


def emu_channel(x32, q, channel, vec, mutant=None, tap=None):
    """one channel in float32, in the kernels' order; `vec`: the 16-byte route (P2 % 4 == 0 and both pointers 16-byte aligned)"""
    x = np.array(x32, np.float32)
    shape = x.shape
    if "blur_sigma" in q:
        w, r = blur_weights(q["blur_sigma"], mutant)
        for ax in range(3):
            n = shape[ax]
            xp = np.take(x, reflect(np.arange(-8, n + 8), n, mutant), axis=ax)
            acc = np.zeros(shape, np.float32)
            for k in range(17):
                acc = _fma32(w[k], np.take(xp, np.arange(k, k + n), axis=ax), acc)
            x = acc
        # the second tile column staged with w0 = 0 and stored at w0 = 128: the tile then holds exactly the H / W pass of columns 0 .. 127 (left
        # reflection included), so column 128 + j receives the finished column j -- which is what copying the finished columns states
        if mutant == "tile_col_w0_zero" and shape[2] > 128:
            x = np.concatenate([x[:, :, :128], x[:, :, :shape[2] - 128]], axis=2)
    if "lowres_zoom" in q:
        tabs = [lowres_axis(shape[ax], q["lowres_zoom"], mutant) for ax in range(3)]
        for ax in (2, 1, 0):
            s0, s1, t, _ = tabs[ax]
            if mutant == "lowres_t_other_axis" and ax == 2:
                t = np.resize(tabs[1][2], t.shape)
            t = t.reshape(_bshape(3, ax))
            x0, x1 = np.take(x, s0, axis=ax), np.take(x, s1, axis=ax)
            x = _fma32(t, (x1 - x0).astype(np.float32), x0)
    noise = None
    if "noise_variance" in q:
        var = float(q["noise_variance"])
        sd = f32(var if mutant == "noise_sd_is_variance" else math.sqrt(var))
        noise = (sd * noise_emu(q["noise_seed"], channel, x.size, mutant, tap).reshape(shape)).astype(np.float32)
    b = f32(q["brightness"]) if "brightness" in q else None
    pre = x
    if mutant == "brightness_before_noise" and b is not None and noise is not None:
        x = (x * b).astype(np.float32) + noise
    else:
        if noise is not None:
            x = x + noise
        if mutant == "contrast_mean_before_brightness":
            pre = x
        if b is not None:
            x = (x * b).astype(np.float32)
    x = x.astype(np.float32)
    gam, con, low = "gamma" in q, "contrast" in q, "lowres_zoom" in q
    first = 0 if con else (1 if gam else 3)
    route = lambda level: vec and not (low and level == first)
    if con:
        mean, _, mn, mx = stats_emu(x, route(0), mutant)
        if mutant == "contrast_mean_before_brightness":
            mean = stats_emu(pre, route(0))[0]
        m, f = f32(mean), f32(q["contrast"])
        x = (((x - m).astype(np.float32) * f).astype(np.float32) + m).astype(np.float32)
        if mutant != "contrast_clip_dropped":
            x = np.minimum(np.maximum(x, f32(mn)), f32(mx))
    if gam:
        inv, retain, g = bool(q.get("gamma_invert")), bool(q.get("gamma_retain_stats")), f32(q["gamma"])
        if mutant == "gamma_min_before_inversion" and inv:
            mean, std, mn, mx = stats_emu(x, route(1), mutant)
            x = -x
        else:
            if inv:
                x = -x
            mean, std, mn, mx = stats_emu(x, route(1), mutant)
        g_min, g_range = f32(mn), f32(mx - mn)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            g_inv = f32(1.0) / (g_range if mutant == "gamma_drop_1e-7" else (g_range + f32(1e-7)))
            t = np.fmax(((x - g_min).astype(np.float32) * g_inv).astype(np.float32), f32(0.0))
            arg = (g * np.log2(t).astype(np.float32)).astype(np.float32)
            if tap is not None:                                # the arguments of v_log_f32 and v_exp_f32
                tap["log2"].append(t)
                tap["exp2"].append(arg)
            p = np.exp2(arg).astype(np.float32)
            y = ((p * g_range).astype(np.float32) + g_min).astype(np.float32)
            if retain:
                ymean, ystd, _, _ = (mean, std, 0, 0) if mutant == "retain_stats_before_gamma" else stats_emu(y, route(2), mutant)
                scale = f32(std / (ystd if ystd >= 1e-8 else 1e-8))
                y = (((y - f32(ymean)).astype(np.float32) * scale).astype(np.float32) + f32(mean)).astype(np.float32)
        x = y if (mutant == "invert_not_undone" or not inv) else -y
    return x.astype(np.float32)


def is_vec(case):
    return case["shape"][2] % 4 == 0 and case["in_off"] % 4 == 0 and case["out_off"] % 4 == 0


def run(case, mode="ref", mutant=None, tap=None, against="device"):
    """mode "ref": dict(out float64 [C, *shape], bar) -- against="host": bar is the tolerance against a float64 side instead; mode "emu": float32 [C, *shape]"""
    x = input_of(case["name"])
    if mode == "emu":
        return np.stack([emu_channel(x[c], q, c, is_vec(case), mutant, tap) for c, q in enumerate(case["params"])])
    outs = [ref_channel(x[c], q, c, against) for c, q in enumerate(case["params"])]
    out = dict(out=np.stack([o for o, _ in outs]), bar=np.stack([b for _, b in outs]))
    out["out"].setflags(write=False)
    out["bar"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(by_name(name))


def worst_ratio(got, want, bar):
    """(max over voxels of |got - want| / bar, with 0 / 0 = 0, x / 0 = inf and a non-finite `got` = inf; index of the worst voxel)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bar)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), np.unravel_index(i, ratio.shape)


# mutant -> the case that shows it (a bar exceeded, or a value no longer finite)
MUTANTS = {
    "blur_unnormalised": "tiles float4",
    "blur_radius_minus_1": "tiles float4",
    "blur_whole_sample_reflect": "tiles float4",
    "tile_col_w0_zero": "tiles float4",
    "lowres_round_src": "tiles float4",
    "lowres_t_other_axis": "tiles scalar",
    "noise_key_ignores_channel": "ragged chunk",
    "noise_swap_z": "ragged chunk",
    "noise_u1_float32": "noise u1 = 1 - 2^-30",
    "noise_sd_is_variance": "ragged chunk",
    "brightness_before_noise": "order",
    "contrast_mean_before_brightness": "order",
    "stats_sample_variance": "offset retain",
    "gamma_drop_1e-7": "grid 2x33x131 C8 tiny",
    "gamma_min_before_inversion": "order",
    "invert_not_undone": "order",
    "retain_stats_before_gamma": "offset retain",
    "stats_drop_last_partial_chunk": "ragged chunk",
    "stats_drop_partials_ge_256": "260 partials",
    "noise_voxel_plus_1": "ragged chunk",
    "contrast_clip_dropped": "contrast clip",
}
# "gamma_drop_1e-7": the issue expected NaN on a constant channel.  That premise does not hold -- 1 / 0 = inf and 0 * inf = NaN, but fmaxf(NaN, 0) = 0 and the
# channel comes out as its minimum, finite and right -- yet the mutant is caught where the range is small against 1e-7: on the tiny family (range 1e-30) t
# becomes (x - min) / range instead of (x - min) 1e7.
# Not listed: "j1 unclamped" -- where j0 is the last coarse sample t is 0 and x0 + 0 (x1 - x0) = x0 for every finite x1 (and the source index is clamped to
# P - 1 as well), so it changes no byte on finite input and no test can tell it from the kernel.


# ---------------------------------------------------------------------------------------------------------------- the exact family
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exact_family(result):
    """bit-level properties of `result(case name) -> float32 [C, *shape]`, premises asserted; the emulation and the device both go through it"""
    for case in cases():                                       # an empty mask copies
        got, x = None, input_of(case["name"])
        for c, q in enumerate(case["params"]):
            if not q:
                got = result(case["name"]) if got is None else got
                assert np.array_equal(bits(got[c]), bits(x[c])), (case["name"], c)
    x, got = input_of("identities"), result("identities")
    q = by_name("identities")["params"]
    assert q[0] == dict(noise_variance=0.0, noise_seed=9) and not (x[0] == 0).any()
    assert np.array_equal(bits(got[0]), bits(x[0])), "variance 0: x + 0 n = x"
    s0, s1, t, nc = lowres_axis(5, 1.0)
    assert q[1] == dict(lowres_zoom=1.0) and nc == 5 and not t.any() and np.array_equal(s0, np.arange(5))
    assert np.array_equal(bits(got[1]), bits(x[1])), "zoom 1: t = 0, s0 = i"
    assert q[2] == dict(lowres_zoom=0.05) and [lowres_axis(n, 0.05)[3] for n in (5, 6, 7)] == [1, 1, 1]
    src = tuple(int(lowres_axis(n, 0.05)[0][0]) for n in (5, 6, 7))
    assert src == (2, 3, 3) and np.array_equal(bits(got[2]), bits(np.full((5, 6, 7), x[2][src], np.float32))), "n_c = 1: the one coarse sample"
    assert q[3] == dict(brightness=1.25)
    assert np.array_equal(bits(got[3]), bits(x[3] * np.float32(1.25))), "brightness alone: the float32 product"
    x, got = input_of("contrast clip"), result("contrast clip")
    for c, f in ((0, 1.25), (2, 0.75), (3, 1.0)):
        assert by_name("contrast clip")["params"][c] == dict(contrast=f)
        assert got[c].min() >= x[c].min() and got[c].max() <= x[c].max(), "the clip bounds are the channel's exact min and max"
        if f > 1:
            assert (got[c] == x[c].max()).any() and (got[c] == x[c].min()).any(), "and for a factor > 1 both are attained"
    x, got = input_of("constant gamma"), result("constant gamma")
    for c, q in enumerate(by_name("constant gamma")["params"]):
        assert np.unique(x[c]).size == 1 and ("gamma" in q or c >= 4)
        assert np.isfinite(got[c]).all(), "a constant channel stays finite through gamma"
        if q.get("gamma_retain_stats") and "blur_sigma" not in q:
            assert np.array_equal(bits(got[c]), bits(x[c])), "and with retain-stats it equals its mean"
    a, b = by_name("align base"), by_name("align in+1")
    assert a["params"] == b["params"] and a["seed"] == b["seed"] and is_vec(a) and not is_vec(b) and a["shape"][2] % 4 == 0
    assert np.array_equal(bits(result("align base")), bits(result("align in+1"))), "the 16-byte route and the scalar route give the same bytes"
    assert np.array_equal(bits(result("align base")), bits(result("align out+1")))
