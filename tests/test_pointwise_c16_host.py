"""The float64 restatements that tests/test_pointwise_c16.py holds the voxel-major pointwise kernels to, the bars of that file, and the proof -- on the CPU
alone -- that (a) the restatements are the reference's operations and (b) the bars can fail.

Restatements: plain numpy float64 on NCDHW arrays -- an einsum over channels, explicit (2z+i, 2y+j, 2x+k) / tap = 4i + 2j + k indexing for the stride-2
gather and scatter, explicit concatenation, explicit where(mask > 0, d, d * slope), and the GroupNorm-backward sums as include/resunet_hip.h /
ru_common.h define them (u = y*k1 + k2, dh = u > thr ? d : d*slope, S1 = sum dh, S2' = sum dh*u per (sample, channel)).  Each is compared here with the
oracle's autograd in double (O.conv1x1x1, O.conv2x2x2_s2, torch.cat, leaky_relu, group_norm) at two small shapes.

Mutants: the four errors this kernel family can make without the network-level bars noticing -- two taps swapped, the LeakyReLU-backward mask on the wrong
half of a split output, S2' summed with d instead of dh, a ragged tail voxel duplicated from voxel V - 1 (the clamp of a ragged tile leaking into the
result) -- are applied to the restatements at the smallest shape of the GPU test they belong to; every one must exceed that test's bar.
Nothing here needs a GPU."""
import numpy as np
import torch

from oracle import resunet_oracle as O

SLOPE = 0.01
TAPS = [(i, j, k) for i in range(2) for j in range(2) for k in range(2)]      # tap = 4i + 2j + k


# ---------------------------------------------------------------------------------------------------------------- bars
def elementwise_excess(got, ref):
    """stored tensors: |d| <= 1e-5 + 1e-5 |ref| (tests/test_hip_ops.py header).  -> max over elements of |d| / bar (<= 1 passes)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))).max())


def relmax_excess(got, ref):
    """reductions over >= 1e3 voxels (weight gradients, statistic sums): max |d| <= 2e-4 max |ref|.  -> max |d| / bar"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (2e-4 * np.abs(ref).max() + 1e-300))


def stats_excess(got, ref, terms):
    """statistic sums [N, C, 2].  `terms` [N, C, V, 2] are the float64 summands.  V >= 1e3: the reduction bar.  Fewer voxels: every summand carries at most the
    elementwise bar of the stored gradient it is made of, so the sum is held to V x (1e-5 + 1e-5 max |summand|), S1 and S2' each with their own summands."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == terms.shape[:2] + (2,), (got.shape, ref.shape, terms.shape)
    nvox = terms.shape[2]
    if nvox >= 1000:
        return max(relmax_excess(got[..., s], ref[..., s]) for s in range(2))
    return max(float(np.abs(got[..., s] - ref[..., s]).max() / (nvox * (1e-5 + 1e-5 * np.abs(terms[..., s]).max()))) for s in range(2))


# ---------------------------------------------------------------------------------------------------------------- restatements
def lrelu(x, slope):
    return np.where(x > 0, x, x * slope)


def finish(y, out_slope=1.0, mask=None, mask_slope=SLOPE, add=None):
    """the store epilogue: LeakyReLU(out_slope), then the LeakyReLU-BACKWARD mask, then the residual"""
    y = lrelu(y, out_slope)
    if mask is not None:
        y = np.where(mask > 0, y, y * mask_slope)
    if add is not None:
        y = y + add
    return y


def ref_conv1(x0, w, x1=None, out_slope=1.0, mask=None, mask_slope=SLOPE, add=None, cout0=0, mask_half=1, dup_tail=False):
    """y[n,o,v] = sum_c w[o,c] cat(x0, x1)[n,c,v]; w [Cout, ldw >= C0 + C1].  cout0 > 0: -> (y, y1) = output channels [:cout0], [cout0:], the mask on y1 only.
    Mutants: mask_half = 0 masks y instead; dup_tail stores voxel V - 1 at voxel V - 2 too."""
    x = np.concatenate([x0, x1], axis=1) if x1 is not None else x0
    y = np.einsum("oc,ncdhw->nodhw", w[:, :x.shape[1]], x)
    if cout0:
        halves = [y[:, :cout0], y[:, cout0:]]
        halves[mask_half] = finish(halves[mask_half], out_slope, mask, mask_slope)
        halves[1 - mask_half] = finish(halves[1 - mask_half], out_slope)
        return halves[0], halves[1]
    y = finish(y, out_slope, mask, mask_slope, add)
    if dup_tail:
        flat = y.reshape(y.shape[0], y.shape[1], -1)
        flat[:, :, -2] = flat[:, :, -1]
    return y


def ref_gather(xf, w5, taps=TAPS):
    """2x2x2 stride-2 convolution: y[n,o,z,y,x] = sum_{c,i,j,k} w5[o,c,i,j,k] xf[n,c,2z+i,2y+j,2x+k].  Mutant: `taps` in another order."""
    wt = w5.reshape(w5.shape[0], w5.shape[1], 8)
    y = 0.0
    for tap, (i, j, k) in enumerate(taps):
        y = y + np.einsum("oc,ncdhw->nodhw", wt[:, :, tap], xf[:, :, i::2, j::2, k::2])
    return y


def ref_scatter(xc, w5, out_slope=1.0, mask=None, mask_slope=SLOPE, add=None, taps=TAPS):
    """its transpose: y[n,c,2z+i,2y+j,2x+k] = sum_o w5[o,c,i,j,k] xc[n,o,z,y,x]; mask / add live on the fine grid"""
    n, _, d, h, w = xc.shape
    wt = w5.reshape(w5.shape[0], w5.shape[1], 8)
    y = np.zeros((n, w5.shape[1], 2 * d, 2 * h, 2 * w))
    for tap, (i, j, k) in enumerate(taps):
        y[:, :, i::2, j::2, k::2] = np.einsum("oc,nodhw->ncdhw", wt[:, :, tap], xc)
    return finish(y, out_slope, mask, mask_slope, add)


def bst_terms(d, bst_y, bst_k, slope=SLOPE, s2_with_d=False, dup_tail=False):
    """summands of the fused GroupNorm-backward statistics of the stored gradient d [N,C,...]: bst_k [N,3,C] = (k1, k2, thr); -> ([N,C,V,2], min |u - thr|).
    Mutants: s2_with_d sums d*u instead of dh*u; dup_tail counts voxel V - 1 twice."""
    n, c = d.shape[:2]
    d, y = d.reshape(n, c, -1), bst_y.reshape(n, c, -1)
    u = y * bst_k[:, 0, :, None] + bst_k[:, 1, :, None]
    thr = bst_k[:, 2, :, None]
    dh = np.where(u > thr, d, d * slope)
    t = np.stack([dh, (d if s2_with_d else dh) * u], axis=-1)
    if dup_tail:
        t = np.concatenate([t, t[:, :, -1:]], axis=2)
    return t, float(np.abs(u - thr).min())


def ref_wgrad1(x, dy, x1=None, dup_tail=False):
    """dw[o,c] = sum_{n,v} dy[n,o,v] cat(x, x1)[n,c,v]"""
    x = np.concatenate([x, x1], axis=1) if x1 is not None else x
    dw = np.einsum("nodhw,ncdhw->oc", dy, x)
    if dup_tail:
        dw = dw + np.einsum("no,nc->oc", dy.reshape(dy.shape[0], dy.shape[1], -1)[:, :, -1], x.reshape(x.shape[0], x.shape[1], -1)[:, :, -1])
    return dw


def ref_wgrad_s2d(xf, dy, taps=TAPS):
    """weight gradient of the stride-2 conv in the reference's layout [Cout, Cin, 2, 2, 2]"""
    dw = np.zeros((dy.shape[1], xf.shape[1], 8))
    for tap, (i, j, k) in enumerate(taps):
        dw[:, :, tap] = np.einsum("nodhw,ncdhw->oc", dy, xf[:, :, i::2, j::2, k::2])
    return dw.reshape(dy.shape[1], xf.shape[1], 2, 2, 2)


def ref_dgrad(dy, w, c0, x1=None, slope=SLOPE, mask_half=1):
    """fused data gradient of the concat 1x1: dx[n,c,v] = sum_o w[o,c] dy[n,o,v]; channels [:c0] -> dx0, the others -> dx1 through the LeakyReLU-backward
    mask of x1 (the activation's output).  Without x1: everything to dx0, no mask.  Mutant: mask_half = 0 masks dx0 instead (equal halves)."""
    cin = c0 + (x1.shape[1] if x1 is not None else 0)
    dx = np.einsum("oc,nodhw->ncdhw", w[:, :cin], dy)
    if x1 is None:
        return dx, None
    dx0, dx1 = dx[:, :c0], dx[:, c0:]
    if mask_half == 1:
        return dx0, np.where(x1 > 0, dx1, dx1 * slope)
    assert x1.shape == dx0.shape
    return np.where(x1 > 0, dx0, dx0 * slope), dx1


# ---------------------------------------------------------------------------------------------------------------- inputs
def draw(seed, *shape, scale=1.0):
    """seeded float32 normal values (what the GPU test feeds the kernels), as a numpy array"""
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(*shape, generator=g) * scale).numpy().astype(np.float32)


def away_from_zero(a, margin=1e-3):
    """mask operands: no |value| below the margin, so that `> 0` cannot be a rounding lottery"""
    a = a.copy()
    small = np.abs(a) < 2 * margin
    a[small] = np.where(a[small] < 0, -2 * margin, 2 * margin).astype(np.float32)
    return a


def draw_bst(seed, n, c, spatial, margin=1e-3):
    """(bst_y [N,C,*spatial], bst_k [N,3,C]) float32 with every |u - thr| >= margin: k1 of both signs (sign(gamma) * rstd), k2 and thr of either sign"""
    y = draw(seed, n, c, *spatial)
    k = draw(seed + 1, n, 3, c)
    k[:, 0] = np.where(k[:, 0] < 0, -1.0, 1.0) * (0.5 + np.abs(k[:, 0]))
    k[:, 1:] *= 0.3
    sh = (n, c) + (1,) * len(spatial)
    k1, k2, thr = (k[:, t].astype(np.float64).reshape(sh) for t in range(3))
    u = y.astype(np.float64) * k1 + k2
    close = np.abs(u - thr) < 2 * margin
    push = np.where(u >= thr, 1.0, -1.0) * 4 * margin / k1
    y = np.where(close, y + push, y).astype(np.float32)
    return y, k


# ---------------------------------------------------------------------------------------------------------------- restatements against the oracle
def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and float(np.abs(a - b).max()) <= tol * (1.0 + float(np.abs(b).max())), float(np.abs(a - b).max())


SMALL_1X1 = [(2, 16, 32, 32, (2, 3, 5), 8), (1, 32, 16, 48, (1, 4, 3), 0)]          # N, C0, C1, Cout, spatial, extra pitch


def test_conv1_restatement_is_the_reference_concat_1x1():
    """forward: O.conv1x1x1 over torch.cat (model.py:424-425), then LeakyReLU (model.py:401-402) and a residual"""
    for si, (n, c0, c1, cout, sp, pad) in enumerate(SMALL_1X1):
        x0, x1, add = (draw(10 * si + t, n, c, *sp).astype(np.float64) for t, c in ((0, c0), (1, c1), (2, cout)))
        w = draw(10 * si + 3, cout, c0 + c1 + pad).astype(np.float64)
        ref = O.leaky_relu(O.conv1x1x1(torch.cat([_t(x0), _t(x1)], 1), _t(w[:, :c0 + c1])[:, :, None, None, None])) + _t(add)
        _close(ref_conv1(x0, w, x1=x1, out_slope=O.LEAKY_SLOPE, add=add), ref.numpy())
        _close(ref_conv1(x0, w[:, :c0]), O.conv1x1x1(_t(x0), _t(w[:, :c0])[:, :, None, None, None]).numpy())


def _concat_1x1_autograd(n, ci, c1, cout, sp, seed):
    """skip, p -> v = leaky_relu(p) -> conv1x1x1(cat(skip, v)) (model.py:422-425), backward of sum(y * dy): -> numpy inputs and the autograd gradients"""
    skip, p, dy = draw(seed, n, ci, *sp), away_from_zero(draw(seed + 1, n, c1, *sp)), draw(seed + 2, n, cout, *sp)
    w = draw(seed + 3, cout, ci + c1)
    ts, tp, tw = _t(skip, True), _t(p, True), _t(w, True)
    v = O.leaky_relu(tp)
    (O.conv1x1x1(torch.cat([ts, v], 1), tw[:, :, None, None, None]) * _t(dy)).sum().backward()
    return dict(skip=skip.astype(np.float64), v=v.detach().numpy(), dy=dy.astype(np.float64), w=w.astype(np.float64),
                dskip=ts.grad.numpy(), dp=tp.grad.numpy(), dw=tw.grad.numpy())


def test_split_output_dgrad_and_weight_gradient_restatements_are_the_reference_backward():
    """the data gradient of the concat 1x1 is (a) a 1x1 with the transposed weight, split output, the LeakyReLU-backward mask of v on the second half, and (b) what
    the fused-dgrad form of the weight gradient writes; the weight gradient is autograd's"""
    for si, (n, ci, c1, cout, sp) in enumerate([(2, 16, 32, 16, (2, 3, 5)), (1, 32, 16, 32, (1, 4, 3))]):
        a = _concat_1x1_autograd(n, ci, c1, cout, sp, 100 + 10 * si)
        y, y1 = ref_conv1(a["dy"], a["w"].T.copy(), mask=a["v"], cout0=ci)
        _close(y, a["dskip"]); _close(y1, a["dp"])
        dx0, dx1 = ref_dgrad(a["dy"], a["w"], ci, x1=a["v"])
        _close(dx0, a["dskip"]); _close(dx1, a["dp"])
        _close(ref_wgrad1(a["skip"], a["dy"], x1=a["v"]), a["dw"])
        _close(ref_dgrad(a["dy"], a["w"][:, :ci], ci)[0], np.einsum("oc,nodhw->ncdhw", a["w"][:, :ci], a["dy"]))


SMALL_S2 = [(2, 16, 32, (1, 2, 3)), (1, 32, 16, (2, 1, 2))]                                 # N, Cin (fine), Cout, coarse extents


def test_stride2_restatements_are_the_reference_conv_and_its_backward():
    for si, (n, cin, cout, (d, h, w)) in enumerate(SMALL_S2):
        xf, w5, dy = draw(200 + si, n, cin, 2 * d, 2 * h, 2 * w), draw(210 + si, cout, cin, 2, 2, 2), draw(220 + si, n, cout, d, h, w)
        tx, tw = _t(xf, True), _t(w5, True)
        y = O.conv2x2x2_s2(tx, tw)
        (y * _t(dy)).sum().backward()
        _close(ref_gather(xf.astype(np.float64), w5.astype(np.float64)), y.detach().numpy())
        _close(ref_scatter(dy.astype(np.float64), w5.astype(np.float64)), tx.grad.numpy())
        _close(ref_wgrad_s2d(xf.astype(np.float64), dy.astype(np.float64)), tw.grad.numpy())


def test_statistics_restatement_is_the_group_norm_backward():
    """z = leaky_relu(group_norm(x)): with k1 = sign(gamma) rstd, k2 = -sign(gamma) mean rstd, thr = -beta / |gamma| (what the engine publishes,
    fin_tail.hpp) the sums are dbeta = S1 and dgamma = sign(gamma) S2' per sample"""
    for si, (n, c, sp) in enumerate([(2, 16, (2, 3, 5)), (1, 32, (3, 2, 2))]):
        x, d = draw(300 + si, n, c, *sp).astype(np.float64), draw(310 + si, n, c, *sp).astype(np.float64)
        gamma = draw(320 + si, c).astype(np.float64) + np.where(np.arange(c) % 2 == 0, 1.0, -1.0) * 2.0
        beta = draw(330 + si, c).astype(np.float64) * 0.3
        cpg = c // O.GN_GROUPS
        xg = x.reshape(n, O.GN_GROUPS, -1)
        mean, rstd = np.repeat(xg.mean(-1), cpg, 1), np.repeat(1.0 / np.sqrt(xg.var(-1) + O.GN_EPS), cpg, 1)
        sg = np.sign(gamma)[None, :]
        k = np.stack([sg * rstd, -sg * mean * rstd, np.broadcast_to((-beta / np.abs(gamma))[None, :], (n, c))], axis=1)
        terms, margin = bst_terms(d, x, k, O.LEAKY_SLOPE)
        assert margin > 1e-6
        sums = terms.sum(2)
        for i in range(n):
            tg, tb = _t(gamma, True), _t(beta, True)
            (O.leaky_relu(O.group_norm(_t(x[i:i + 1]), tg, tb)) * _t(d[i:i + 1])).sum().backward()
            _close(sums[i, :, 0], tb.grad.numpy(), 1e-9)
            _close(sums[i, :, 1] * np.sign(gamma), tg.grad.numpy(), 1e-9)


def test_input_generators_keep_the_mask_decisions_off_the_rounding_edge():
    y, k = draw_bst(5, 2, 32, (1, 1, 63))
    assert y.dtype == np.float32 and k.dtype == np.float32 and (k[:, 0] < 0).any() and (k[:, 0] > 0).any()
    _, margin = bst_terms(np.ones(y.shape), y.astype(np.float64), k.astype(np.float64))
    assert margin >= 1e-3
    m = away_from_zero(draw(6, 2, 16, 1, 1, 63))
    assert m.dtype == np.float32 and float(np.abs(m).min()) >= 1e-3 and (m < 0).any()


# ---------------------------------------------------------------------------------------------------------------- mutants
SWAP = [TAPS[1], TAPS[0]] + TAPS[2:]                                                      # the two x taps of (i, j) = (0, 0) change places


def test_mutants_exceed_the_bars_of_the_gpu_tests():
    """each at the smallest shape of the GPU test it belongs to (tests/test_pointwise_c16.py: GATHER[0], SCATTER[0], SPLIT[0], PLAIN V = 63, PLAIN_BST V = 63,
    WGRAD V = 1, WGRAD_S2D 2x3x8, DGRAD 105 voxels); float32-drawn inputs as on the device.  The unmutated restatement has excess 0 by construction."""
    f8 = lambda a: a.astype(np.float64)
    rows = []
    # two taps swapped: gather 1x1x1 coarse, 128 -> 32; scatter 32 -> 128 at 2x3x8; stride-2 weight gradient 128 -> 32 at 2x3x8
    xf, w5 = f8(draw(1, 1, 16, 2, 2, 2)), f8(draw(2, 32, 16, 2, 2, 2, scale=128 ** -0.5))
    rows.append(("taps swapped, gather", elementwise_excess(ref_gather(xf, w5, SWAP), ref_gather(xf, w5))))
    xc, w5 = f8(draw(3, 1, 32, 2, 3, 8)), f8(draw(4, 32, 16, 2, 2, 2, scale=32 ** -0.5))
    rows.append(("taps swapped, scatter", elementwise_excess(ref_scatter(xc, w5, taps=SWAP), ref_scatter(xc, w5))))
    by, bk = (f8(a) for a in draw_bst(5, 1, 16, (4, 6, 16)))
    good, _ = bst_terms(ref_scatter(xc, w5), by, bk)
    bad, _ = bst_terms(ref_scatter(xc, w5, taps=SWAP), by, bk)
    rows.append(("taps swapped, scatter statistics", stats_excess(bad.sum(2), good.sum(2), good)))
    xf, dy = f8(draw(6, 1, 16, 4, 6, 16)), f8(draw(7, 1, 32, 2, 3, 8))
    rows.append(("taps swapped, stride-2 weight gradient", relmax_excess(ref_wgrad_s2d(xf, dy, SWAP), ref_wgrad_s2d(xf, dy))))
    # mask on the wrong half: split output (16, 32) at V = 63; fused data gradient 16 + 16 <- 16 at 105 voxels
    x, w, m = f8(draw(8, 1, 16, 1, 1, 63)), f8(draw(9, 32, 16, scale=0.25)), f8(away_from_zero(draw(10, 1, 16, 1, 1, 63)))
    good, bad = ref_conv1(x, w, mask=m, cout0=16), ref_conv1(x, w, mask=m, cout0=16, mask_half=0)
    rows.append(("mask on the wrong half, split output", max(elementwise_excess(b, g) for b, g in zip(bad, good))))
    dy, w, x1 = f8(draw(11, 2, 16, 3, 5, 7)), f8(draw(12, 16, 32, scale=0.25)), f8(away_from_zero(draw(13, 2, 16, 3, 5, 7)))
    good, bad = ref_dgrad(dy, w, 16, x1), ref_dgrad(dy, w, 16, x1, mask_half=0)
    rows.append(("mask on the wrong half, fused data gradient", max(elementwise_excess(b, g) for b, g in zip(bad, good))))
    # S2' summed with d instead of dh: plain mode, 16 channels, V = 63
    d = ref_conv1(f8(draw(14, 1, 16, 1, 1, 63)), f8(draw(15, 16, 16, scale=0.25)))
    by, bk = (f8(a) for a in draw_bst(16, 1, 16, (1, 1, 63)))
    good, _ = bst_terms(d, by, bk)
    rows.append(("S2' of d instead of dh", stats_excess(bst_terms(d, by, bk, s2_with_d=True)[0].sum(2), good.sum(2), good)))
    # a ragged tail voxel duplicated from V - 1: stored output and statistics at V = 63, weight gradient at V = 1
    x, w = f8(draw(14, 1, 16, 1, 1, 63)), f8(draw(15, 16, 16, scale=0.25))
    rows.append(("tail voxel duplicated, stored output", elementwise_excess(ref_conv1(x, w, dup_tail=True), ref_conv1(x, w))))
    rows.append(("tail voxel duplicated, statistics", stats_excess(bst_terms(d, by, bk, dup_tail=True)[0].sum(2), good.sum(2), good)))
    x, dy = f8(draw(17, 1, 16, 1, 1, 1)), f8(draw(18, 1, 16, 1, 1, 1))
    rows.append(("tail voxel duplicated, weight gradient", relmax_excess(ref_wgrad1(x, dy, dup_tail=True), ref_wgrad1(x, dy))))
    for name, ex in rows:
        print("  mutant %-46s error / bar %.3g" % (name, ex))
    for name, ex in rows:
        assert ex > 1.0, (name, ex)
