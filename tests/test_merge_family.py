"""The one merge family of csrc/ensemble.hip (merge_kernel, finalize_kernel, merge_epilogue, paste_kernel) where a lane takes four voxels: what the
one-voxel-per-lane kernels it replaced never met.  Everything is called through the C ABI and compared bit for bit with the restatements that exist:
test_scalar_passes_host.ref_merge / box_of for a model's un-flipped mean, inference.ensemble_mean_host / ensemble_merge_host across models, numpy for the paste.

  quad tails and narrow rows   boxes with Vb % 4 = 0, 1, 2, 3 and rows shorter than, equal to and longer than a quad, inside padding that holds values near 8;
                               ru_tta_merge_box and ru_ens_accumulate (two models) + ru_ens_finalize, C = 1 and 4, K = 1 and 8 (every flip code at K = 8)
  misaligned pointers          the same calls with probs / acc / mean 4 bytes off a 16-byte boundary, and with mask 1 byte off a 4-byte boundary (the bytewise store):
                               the outputs of the aligned run, guards on both sides untouched
  the identities               ru_tta_merge = ru_tta_merge_box on the whole box = ru_ens_accumulate_finalize(first, M = 1) = the first three outputs of
                               ru_unc_accumulate_finalize for both measures
  NaN and exactly 1/2          mask 0 at both, counts as numpy's, the mean NaN where numpy's is
  paste                        ru_paste_labels, ru_paste_u8c, ru_paste_probs against zero-fill-and-assign, W % 4 == 0 and not, destination 1 byte off alignment

Outputs lie between GUARD bytes of 0xA5 on either side (tests/test_scalar_passes.py's filled / inner, here with a byte offset), which every read checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_scalar_passes_host as H
from brats2019_amd import inference as I
from op_cases import PATTERN

pytestmark = pytest.mark.gpu
GUARD = 32

# (box size, box lo, volume): Vb % 4 = 0, 1, 2, 3, 0, 0; box rows of 5, 9, 7, 7, 3 and 1 voxels
BOXES = [((3, 4, 5), (1, 1, 1), (5, 6, 7)), ((3, 7, 9), (2, 0, 5), (6, 7, 18)), ((5, 6, 7), (0, 0, 0), (5, 6, 7)), ((3, 3, 7), (1, 1, 1), (4, 5, 9)),
         ((4, 2, 3), (0, 1, 0), (4, 3, 3)), ((3, 4, 1), (0, 0, 3), (3, 4, 6))]
FLIPS = {1: H.MERGE_FLIPS[1], 8: H.MERGE_FLIPS[8]}
MODELS = 2


@pytest.fixture(scope="module")
def lib():
    from brats2019_amd import _lib as L
    L.require_gpu()
    return L.load()


def call(lib, name, *args):
    from brats2019_amd import _lib as L
    L.check(getattr(lib, name)(*args), name)


def stream():
    from brats2019_amd import _lib as L
    return L.stream()


def ints3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


class Buf:
    """n elements of `dtype` on the device, `skew` bytes past a 16-byte boundary, between GUARD bytes of PATTERN; `a` fills them (an input)"""

    def __init__(self, n, dtype, skew=0, a=None):
        self.n, self.dtype, self.off = int(n), np.dtype(dtype), GUARD + skew
        host = np.full(self.off + self.n * self.dtype.itemsize + GUARD, PATTERN, np.uint8)
        if a is not None:
            host[self.off:self.off + self.n * self.dtype.itemsize] = np.ascontiguousarray(a, self.dtype).reshape(-1).view(np.uint8)
        self.raw = torch.from_numpy(host).cuda()
        assert self.raw.data_ptr() % 16 == 0 and GUARD % 16 == 0

    @property
    def p(self):
        return C.c_void_p(self.raw.data_ptr() + self.off)

    def get(self):
        h = self.raw.cpu().numpy()
        end = self.off + self.n * self.dtype.itemsize
        assert (h[:self.off] == PATTERN).all() and (h[end:] == PATTERN).all(), "guard bytes overwritten"
        return h[self.off:end].copy().view(self.dtype)


def padded_inputs(k, c, size, lo, vol, flips, seed):
    """probs [K, C, *vol] float32: un-flipped, copy k is uniform in [0, 1) inside the box and in [7, 8) in the padding, so a read outside the box shows"""
    rng = np.random.RandomState(seed)
    u = (7.0 + rng.rand(k, c, *vol)).astype(np.float32)
    u[:, :, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = rng.rand(k, c, *size).astype(np.float32)
    return np.stack([np.ascontiguousarray(np.flip(u[i], H._axes(f))) if f else u[i] for i, f in enumerate(flips)])


def run_tta_box(lib, probs, flips, lo, size, f4=0, u1=0):
    k, c, d, h, w = probs.shape
    vb = int(np.prod(size))
    src, mean, mask, counts = Buf(probs.size, np.float32, f4, probs), Buf(c * vb, np.float32, f4), Buf(c * vb, np.uint8, u1), Buf(c, np.int64)
    call(lib, "ru_tta_merge_box", src.p, k, H.flips_word(flips), mean.p, mask.p, counts.p, c, d, h, w, ints3(lo), ints3(size), stream())
    src.get()
    return mean.get(), mask.get(), counts.get()


def run_ens(lib, models, flips, lo, size, f4=0, u1=0):
    """ru_ens_accumulate per model, then ru_ens_finalize: (mean, mask, counts, the stored sum)"""
    k, c, d, h, w = models[0].shape
    vb = int(np.prod(size))
    acc, mean, mask, counts = Buf(c * vb, np.float32, f4), Buf(c * vb, np.float32, f4), Buf(c * vb, np.uint8, u1), Buf(c, np.int64)
    for m, probs in enumerate(models):
        src = Buf(probs.size, np.float32, f4, probs)
        call(lib, "ru_ens_accumulate", src.p, k, H.flips_word(flips), acc.p, int(m == 0), c, d, h, w, ints3(lo), ints3(size), stream())
        src.get()
    call(lib, "ru_ens_finalize", acc.p, len(models), mean.p, mask.p, counts.p, c, vb, stream())
    return mean.get(), mask.get(), counts.get(), acc.get()


def reference(models, flips, lo, size):
    per_model = [H.box_of(H.ref_merge(p, flips)[0], lo, size) for p in models]
    out = []
    for group in (per_model[:1], per_model):                          # the TTA merge of the first model, the ensemble of all
        mean = I.ensemble_mean_host(group)
        mask = (mean > 0.5).astype(np.uint8)
        out.append((mean.reshape(-1), mask.reshape(-1), mask.reshape(mask.shape[0], -1).sum(1).astype(np.int64)))
    total = per_model[0]
    for p in per_model[1:]:
        total = total + p
    return out[0], out[1], total.reshape(-1)


def same(got, ref):
    return (np.array_equal(H.bits32(got[0]), H.bits32(ref[0])), np.array_equal(got[1], ref[1]), np.array_equal(got[2], ref[2]))


CASES = [(box, c, k) for box in BOXES for c in (1, 4) for k in (1, 8)]


def case_id(case):
    (size, lo, vol), c, k = case
    return "%s_at_%s_in_%s_C%d_K%d" % ("x".join(map(str, size)), "x".join(map(str, lo)), "x".join(map(str, vol)), c, k)


@pytest.fixture(scope="module")
def merge_case():
    """inputs, references and the aligned device run of a case, made once and shared by the tests below"""
    cache = {}

    def get(lib, case):
        if case not in cache:
            (size, lo, vol), c, k = case
            models = [padded_inputs(k, c, size, lo, vol, FLIPS[k], 1000 * m + 7 * c + k + sum(vol)) for m in range(MODELS)]
            ref_tta, ref_ens, ref_sum = reference(models, FLIPS[k], lo, size)
            cache[case] = (models, ref_tta, ref_ens, ref_sum, run_tta_box(lib, models[0], FLIPS[k], lo, size), run_ens(lib, models, FLIPS[k], lo, size))
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_quad_tails_and_narrow_rows(case, lib, merge_case):
    models, ref_tta, ref_ens, ref_sum, tta, ens = merge_case(lib, case)
    assert 0 < ref_ens[2].min() and ref_ens[2].max() < int(np.prod(case[0][0])), "the masks are neither empty nor full"
    assert all(same(tta, ref_tta)), ("ru_tta_merge_box: mean / mask / counts equal", same(tta, ref_tta))
    assert np.array_equal(H.bits32(ens[3]), H.bits32(ref_sum)), "ru_ens_accumulate: the stored sum"
    assert all(same(ens, ref_ens)), ("ru_ens_accumulate + ru_ens_finalize: mean / mask / counts equal", same(ens, ref_ens))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_misaligned_pointers_give_the_aligned_outputs(case, lib, merge_case):
    (size, lo, vol), c, k = case
    models, _, _, _, tta, ens = merge_case(lib, case)
    for f4, u1 in ((4, 0), (0, 1)):
        got = run_tta_box(lib, models[0], FLIPS[k], lo, size, f4, u1)
        assert all(same(got, tta)), ("ru_tta_merge_box", f4, u1, same(got, tta))
        got = run_ens(lib, models, FLIPS[k], lo, size, f4, u1)
        assert all(same(got, ens)) and np.array_equal(H.bits32(got[3]), H.bits32(ens[3])), ("ru_ens_accumulate + ru_ens_finalize", f4, u1, same(got, ens))


def as_bits(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.float32 else a)


def test_the_identities_of_the_family(lib):
    size, lo, vol = BOXES[1]
    c, k = 4, 8
    d, h, w = vol
    probs = padded_inputs(k, c, size, lo, vol, FLIPS[k], 4242)
    word, src = H.flips_word(FLIPS[k]), Buf(probs.size, np.float32, 0, probs)
    for blo, bsize in ((lo, size), ((0, 0, 0), vol)):
        vb = int(np.prod(bsize))
        rows = {"ru_tta_merge_box": run_tta_box(lib, probs, FLIPS[k], blo, bsize)}
        if bsize == vol:
            mean, mask, counts = Buf(c * vb, np.float32), Buf(c * vb, np.uint8), Buf(c, np.int64)
            call(lib, "ru_tta_merge", src.p, k, word, mean.p, mask.p, counts.p, c, d, h, w, stream())
            rows["ru_tta_merge"] = (mean.get(), mask.get(), counts.get())
        mean, mask, counts = Buf(c * vb, np.float32), Buf(c * vb, np.uint8), Buf(c, np.int64)
        call(lib, "ru_ens_accumulate_finalize", src.p, k, word, None, 1, 1, mean.p, mask.p, counts.p, c, d, h, w, ints3(blo), ints3(bsize), stream())
        rows["ru_ens_accumulate_finalize"] = (mean.get(), mask.get(), counts.get())
        for measure in (0, 1):                                            # RU_UNC_STD, RU_UNC_ENTROPY
            mean, mask, counts, unc = Buf(c * vb, np.float32), Buf(c * vb, np.uint8), Buf(c, np.int64), Buf(c * vb, np.uint8)
            call(lib, "ru_unc_accumulate_finalize", src.p, k, word, None, None, 1, 1, measure, mean.p, mask.p, counts.p, unc.p, c, d, h, w, ints3(blo),
                 ints3(bsize), stream())
            rows["ru_unc_accumulate_finalize measure %d" % measure] = (mean.get(), mask.get(), counts.get())
            assert unc.get().max() <= 100
        first = rows["ru_tta_merge_box"]
        ref = H.ref_merge(probs, FLIPS[k])
        rm, rk = H.box_of(ref[0], blo, bsize).reshape(-1), H.box_of(ref[1], blo, bsize).reshape(-1)
        assert all(same(first, (rm, rk, rk.reshape(c, -1).sum(1).astype(np.int64))))
        for name, got in rows.items():
            for a, b in zip(got, first):                                  # mean (by bit pattern), mask, counts
                assert torch.equal(as_bits(a), as_bits(b)), name
    src.get()


def test_a_nan_and_an_exact_half(lib):
    size, lo, vol = BOXES[1]
    c, k = 3, len(I.TTA_FLIPS)
    flips = [sum({1: 1, 2: 2, 3: 4}[ax] for ax in axes) for axes in I.TTA_FLIPS]
    probs = padded_inputs(k, c, size, lo, vol, [0] * k, 99)              # un-flipped still
    at_nan, at_half = (lo[0] + 1, lo[1] + 3, lo[2] + 4), (lo[0] + 2, lo[1] + 6, lo[2] + 8)
    probs[2][(slice(None),) + at_nan] = np.nan                           # in one copy
    probs[(slice(None), slice(None)) + at_half] = 0.5                    # in every copy: the mean is exactly 1/2
    probs = np.stack([np.ascontiguousarray(np.flip(probs[i], axes)) if axes else probs[i] for i, axes in enumerate(I.TTA_FLIPS)])
    rmean, rmask, rcounts = I.ensemble_merge_host([probs], pad_left=lo, size=size)
    in_nan, in_half = tuple(a - b for a, b in zip(at_nan, lo)), tuple(a - b for a, b in zip(at_half, lo))
    assert np.isnan(rmean[(slice(None),) + in_nan]).all() and int(np.isnan(rmean).sum()) == c and (rmean[(slice(None),) + in_half] == 0.5).all()
    d, h, w = vol
    vb = int(np.prod(size))
    src = Buf(probs.size, np.float32, 0, probs)
    mean, mask, counts, unc = Buf(c * vb, np.float32), Buf(c * vb, np.uint8), Buf(c, np.int64), Buf(c * vb, np.uint8)
    call(lib, "ru_unc_accumulate_finalize", src.p, k, H.flips_word(flips), None, None, 1, 1, 0, mean.p, mask.p, counts.p, unc.p, c, d, h, w, ints3(lo), ints3(size),
         stream())
    for got in (run_tta_box(lib, probs, flips, lo, size), run_ens(lib, [probs], flips, lo, size)[:3], (mean.get(), mask.get(), counts.get())):
        gmean, gmask = got[0].reshape(rmean.shape), got[1].reshape(rmean.shape)
        assert not gmask[(slice(None),) + in_nan].any() and not gmask[(slice(None),) + in_half].any()
        assert np.array_equal(gmask, rmask.astype(np.uint8)) and np.array_equal(got[2], np.asarray(rcounts, np.int64))
        assert np.array_equal(np.isnan(gmean), np.isnan(rmean))
        ok = ~np.isnan(rmean)
        assert np.array_equal(H.bits32(gmean[ok]), H.bits32(rmean[ok]))


# ---------------------------------------------------------------------------------------------------------------- paste
def paste_boxes(vol):
    d, h, w = vol
    return [((1, 1, 1), (max(1, d - 2), max(1, h - 2), max(1, w - 2))),     # inside
            ((0, 1, w - 3), (d - 1, h - 2, 3)),                              # touching the z = 0 and the x = W - 1 faces
            ((0, 0, 0), vol)]


@pytest.mark.parametrize("vol", [(5, 6, 7), (5, 6, 8), (2, 3, 4)], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("c", [1, 3])
def test_paste_is_zero_fill_and_assign(vol, c, lib):
    d, h, w = vol
    rng = np.random.RandomState(d * 100 + w * 10 + c)
    for lo, size in paste_boxes(vol):
        sl = (slice(None), slice(lo[0], lo[0] + size[0]), slice(lo[1], lo[1] + size[1]), slice(lo[2], lo[2] + size[2]))
        entries = [("ru_paste_u8c", np.uint8), ("ru_paste_probs", np.float32)] + ([("ru_paste_labels", np.uint8)] if c == 1 else [])
        for name, dtype in entries:
            box = (1 + rng.randint(0, 250, size=(c,) + tuple(size))).astype(dtype)                      # never 0: every box voxel shows
            ref = np.zeros((c,) + vol, dtype)
            ref[sl] = box
            for skew in ((0, 1) if dtype == np.uint8 else (0, 4)):
                src, full = Buf(box.size, dtype, 0, box), Buf(ref.size, dtype, skew)
                args = (src.p, full.p) + ((c,) if name != "ru_paste_labels" else ()) + (d, h, w, ints3(lo), ints3(size), stream())
                call(lib, name, *args)
                assert np.array_equal(full.get().reshape(ref.shape), ref), (name, vol, c, lo, size, skew)
