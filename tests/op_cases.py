"""What tests/test_op_workspace.py and tools/op_abi_bytes.py share: one case per op-level entry that takes a workspace and per branch of its carve, on
seeded inputs, at the smallest shapes the other suites use to reach those branches.  A case is (name, short, run): run() calls the entry through
brats2019_amd.ops -- which sizes the workspace with the entry's query and allocates it with _lib.workspace -- and returns its output tensors; short says
that the query is ONE walk that takes something, so that a workspace one 256-byte unit below it must be refused.  GuardedWorkspace stands in for
_lib.workspace and decides how many bytes the entry really gets, with a guard behind them."""
import torch

GUARD = 4096
PATTERN = 0xA5


class GuardedWorkspace:
    """_lib.workspace(nbytes, device) -> the first size_of(nbytes) bytes of an allocation that goes on for GUARD bytes of PATTERN"""

    def __init__(self, size_of=lambda nbytes: nbytes):
        self.size_of, self.bufs = size_of, []

    def __call__(self, nbytes, device):
        n = max(int(self.size_of(int(nbytes))), 0)
        buf = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=device)       # (stale workspace bytes read as NaN)
        buf[n:] = PATTERN
        self.bufs.append((buf, n))
        return buf[:n]

    def intact(self):
        torch.cuda.synchronize()
        return len(self.bufs) > 0 and all(bool((buf[n:] == PATTERN).all()) for buf, n in self.bufs)


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _c16(n, c, d, h, w, seed):
    return _rand(n, c // 16, d, h, w, 16, seed=seed)


def cases():
    from brats2019_amd import ops
    out = []
    add = lambda name, short, run: out.append((name, short, run))
    as_list = lambda r: [t for t in (r if isinstance(r, (tuple, list)) else (r,)) if isinstance(t, torch.Tensor)]

    # ---- ru_conv3d_fwd_p / _bwd_data_p / _bwd_weight_p, k = 1, 2, 3: 1 x 8 -> 8 at 8 x 8 x 8 (one query serves all of them: no short case)
    n, c, s = 1, 8, 8
    for k in (1, 2, 3):
        for prec in (("f32", "bf16x3") if k == 3 else ("f32",)):
            x, w = _rand(n, c, s, s, s, seed=10 + k), _rand(c, c, k, k, k, seed=20 + k, scale=0.2)
            so = s // 2 if k == 2 else s
            dy, b = _rand(n, c, so, so, so, seed=30 + k), (_rand(c, seed=40) if k == 3 else None)
            add("conv3d_fwd_k%d_%s" % (k, prec), False, lambda x=x, w=w, b=b, prec=prec: as_list(ops.conv3d(x, w, b, precision=prec)))
            add("conv3d_bwd_data_k%d_%s" % (k, prec), False, lambda dy=dy, w=w, prec=prec: as_list(ops.conv3d_bwd_data(dy, w, (s, s, s), precision=prec)))
            add("conv3d_bwd_weight_k%d_%s" % (k, prec), False, lambda x=x, dy=dy, k=k, prec=prec: as_list(ops.conv3d_bwd_weight(x, dy, k, with_bias=(k == 3), precision=prec)))

    # ---- ru_conv3d_fwd_splitk, 1 x 32 -> 32 at 4 x 4 x 16 (tests/test_ncdhw_convs_host.py): the packed weight and two partial tensors; the factor chosen and given
    xk, wk = _rand(1, 32, 4, 4, 16, seed=45), _rand(32, 32, 3, 3, 3, seed=46, scale=0.05)
    add("conv3d_fwd_splitk", True, lambda: as_list(ops.conv3d_splitk(xk, wk)))
    add("conv3d_fwd_splitk_given", True, lambda: as_list(ops.conv3d_splitk(xk, wk, ksplit=2)))

    # ---- GroupNorm: N = 1, C = 16, V = 8192 + 1 -- two tiles
    x, dy = _rand(1, 16, 1, 1, 8193, seed=50), _rand(1, 16, 1, 1, 8193, seed=51)
    gamma, beta = _rand(16, seed=52) + 1.0, _rand(16, seed=53)

    def gn_bwd():
        _, mean, rstd = ops.group_norm(x, gamma, beta, slope=0.01)
        return as_list(ops.group_norm_bwd(x, gamma, beta, mean, rstd, dy, slope=0.01))
    add("groupnorm_fwd", False, lambda: as_list(ops.group_norm(x, gamma, beta, slope=0.01, residual=dy)))
    add("groupnorm_bwd", False, gn_bwd)

    # ---- the 3x3x3 layout launch, 1 x 16 -> 16 at 8 x 8 x 16: plain, split-form input, exact f32, activations; bit 6 where the shape does not take it
    n, d, h, w_ = 1, 8, 8, 16
    xv, xn = _c16(n, 16, d, h, w_, seed=60), _rand(n, 16, d, h, w_, seed=61)
    wt, bias = _rand(16, 16, 3, 3, 3, seed=62, scale=0.1), _rand(16, seed=63)
    for tag, kw in (("ncdhw", {}), ("in16", dict(in_c16=True)), ("out16", dict(out_c16=True)), ("c16", dict(in_c16=True, out_c16=True)),
                    ("c16_split", dict(in_c16=True, out_c16=True, in_split=True)), ("c16_f32", dict(in_c16=True, out_c16=True, exact_f32=True)),
                    ("c16_act", dict(in_c16=True, out_c16=True, activations=True)), ("c16_grad_small", dict(in_c16=True, out_c16=True, gradient=True))):
        xin = (ops.to_split_c16(xv) if kw.get("in_split") else xv) if kw.get("in_c16") else xn
        add("conv3_l_" + tag, True, lambda xin=xin, kw=kw: as_list(ops.conv3_fused(xin, wt, **kw).y))
        add("conv3d_fwd_l_" + tag, True, lambda xin=xin, kw=kw: as_list(ops.conv3d_layout(xin, wt, **kw)))
    add("conv3_l_c16_bias", True, lambda: as_list(ops.conv3_fused(xv, wt, bias=bias, in_c16=True, out_c16=True).y))
    add("conv3d_bwd_weight_l_ncdhw", False, lambda: as_list(ops.conv3d_bwd_weight_layout(xn, xn)))
    add("conv3d_bwd_weight_l_c16", False, lambda: as_list(ops.conv3d_bwd_weight_layout(xv, xv, x_c16=True, dy_c16=True)))
    # flag bit 2, the 4-channel copy: 2 x 4 -> 16 at 32 x 32 x 64 (the shape must fit the 4-channel kernel)
    x4, w4 = _rand(2, 4, 32, 32, 64, seed=64), _rand(16, 4, 3, 3, 3, seed=65, scale=0.2)
    for tag, kw in (("c4_out16", dict(few_channels=True, out_c16=True)), ("c4", dict(few_channels=True))):
        add("conv3_l_" + tag, True, lambda kw=kw: as_list(ops.conv3_fused(x4, w4, **kw).y))
        add("conv3d_fwd_l_" + tag, True, lambda kw=kw: as_list(ops.conv3d_layout(x4, w4, **kw)))
    # flag bit 6, the gradient-operand tensor: 2 x 16 -> 16 at 30 x 44 x 40
    xg = _c16(2, 16, 30, 44, 40, seed=66)
    add("conv3_l_c16_grad", True, lambda: as_list(ops.conv3_fused(xg, wt, in_c16=True, out_c16=True, gradient=True).y))
    add("conv3d_fwd_l_c16_grad", True, lambda: as_list(ops.conv3d_layout(xg, wt, in_c16=True, out_c16=True, gradient=True)))

    # ---- one launch per route family of the 3x3x3 split-bf16 kernels (each reads another form of the weight pack), at the smallest shapes
    # tests/test_conv3_fused_host.py lists for them
    s60 = (30, 30, 60)
    x32, w32 = _c16(2, 32, 32, 32, 32, seed=100), _rand(32, 32, 3, 3, 3, seed=101, scale=0.06)
    x32r = _c16(2, 32, 32, 30, 44, seed=102)
    x16, a16 = _c16(2, 16, *s60, seed=103), _c16(2, 16, *s60, seed=104)
    sc16, sh16 = _rand(2, 16, seed=105) + 1.5, _rand(2, 16, seed=106, scale=0.5)
    w3, b3 = _rand(3, 16, 3, 3, 3, seed=107, scale=0.1), _rand(3, seed=108)
    xs24, as24 = _c16(1, 16, 8, 16, 18, seed=109), _c16(1, 16, 8, 16, 18, seed=110)
    for tag, want, xin, wgt, kw in (
            ("wz32", ("wz32", False, False), x32, w32, dict(in_c16=True, out_c16=True)),
            ("wz32mx", ("wz32mx", False, False), x32r, w32, dict(in_c16=True, out_c16=True, activations=True)),
            ("mx_fwd", ("mx", False, False), x16, wt, dict(in_c16=True, out_c16=True, activations=True)),
            ("mx_grad", ("mx", False, True), x16, wt, dict(in_c16=True, out_c16=True, gradient=True, weight_mode=1)),
            ("head", ("sb2", True, False), x16, w3, dict(in_c16=True, bias=b3, sigmoid=True)),
            ("head_res", ("sb2", True, False), x16, w3, dict(in_c16=True, bias=b3, sigmoid=True, in_scale=sc16, in_shift=sh16, in_res=a16, in_sum_out=True)),
            ("sb2_add", ("sb2", False, False), x16, wt, dict(in_c16=True, out_c16=True, add=a16, stats=True)),
            ("sb_add", ("sb", False, False), xs24, wt, dict(in_c16=True, out_c16=True, add=as24, stats=True))):
        def run(xin=xin, wgt=wgt, kw=kw, want=want):
            r = ops.conv3_fused(xin, wgt, **kw)
            route = ops.conv3_route(r.route)
            assert (route.family, route.head, route.grad) == want, (want, route)
            return as_list([r.y, r.in_sum, r.partials])
        add("conv3_l_route_" + tag, True, run)

    # ---- the in-launch tail of ru_conv3_l (flag bit 8 of the query: the ticket) and ru_gn_bwd_l (partials, coefficients, ticket): a guarded workspace arrives
    # filled with 0xFF, so the ticket these entries zero on the stream is part of what the cases check
    gam16, bet16 = _rand(16, seed=111) + 1.0, _rand(16, seed=112)
    mean16, rstd16 = _rand(16, seed=113, scale=0.3), _rand(16, seed=114, scale=0.1) + 1.0

    def conv3_tail():
        r = ops.conv3_fused(xs24, wt, in_c16=True, out_c16=True, add=as24, stats=True, tail=1, tail_gamma=gam16, tail_beta=bet16, tail_want_k=True)
        return as_list([r.y, r.partials] + list(r.fin[0]))
    add("conv3_l_tail", True, conv3_tail)
    xg5, dg5 = _c16(2, 16, 1, 3, 683, seed=115), _c16(2, 16, 1, 3, 683, seed=116)          # V = 2049: five partials per (sample, channel)
    for tag, kw in (("", {}), ("_tail", dict(tail=True)), ("_tail_split", dict(tail=True, split=True)), ("_stop", dict(stop_after_finalize=True))):
        add("gn_bwd_l" + tag, True, lambda kw=kw: as_list(ops.gn_bwd_c16(xg5, dg5, gam16, sc16, sh16, mean16, rstd16, 0.01, **kw)))

    # ---- ru_head_grad_l, one case per route: 2 x 3 classes at V = 16384 + 4 (two bias partials per row; the generic route at V = 16384 + 1)
    ph, dph = torch.sigmoid(_rand(2, 3, 16388, seed=120, scale=3.0)), _rand(2, 3, 16388, seed=121)
    gh = (_rand(2, 3, 16388, seed=122) > 0.5).float()
    add("head_grad_l_c4", True, lambda: as_list(ops.head_grad(ph, dph, with_dlog=True)))
    sh = ops.criterion_sums(ph, gh)                      # (taken here: the criterion's own workspace is not what the case is about)
    add("head_grad_l_crit", True, lambda: as_list(ops.head_grad(ph, target=gh, sums=sh, count=3 * ph.numel())))
    add("head_grad_l_generic", True, lambda: as_list(ops.head_grad(ph[..., :16385], dph[..., :16385], generic=True)))

    # ---- ru_conv1_l: plain (takes nothing), gather and scatter of 1 x 16 -> 32 at one coarse voxel
    xf, xc = _c16(1, 16, 2, 2, 2, seed=70), _c16(1, 32, 1, 1, 1, seed=71)
    wg, wsc, wp = _rand(32, 16, 2, 2, 2, seed=72, scale=0.3), _rand(32, 16, 2, 2, 2, seed=73, scale=0.3), _rand(32, 16, seed=74, scale=0.3)
    add("conv1_l_plain", False, lambda: as_list(ops.conv1x1_c16(xf, wp).y))
    add("conv1_l_gather", True, lambda: as_list(ops.conv1x1_c16(xf, wg, s2d=1).y))
    add("conv1_l_scatter", True, lambda: as_list(ops.conv1x1_c16(xc, wsc, s2d=2).y))
    # ---- ru_wgrad1_l: 1 x 16 -> 32
    x1, dy1 = _c16(1, 16, 2, 3, 5, seed=75), _c16(1, 32, 2, 3, 5, seed=76)
    add("wgrad1_l", True, lambda: as_list(ops.conv1x1_bwd_weight_c16(x1, dy1).dw))

    # ---- ru_wgrad3_l at the ragged shape of tests/test_wgrad3_fused_host.py (RAG): plain, x as a 4-channel copy, dy as a 4-channel copy, deferred reduction
    n, (d, h, w_) = 2, (5, 11, 19)
    x3, dy3 = _c16(n, 16, d, h, w_, seed=80), _c16(n, 16, d, h, w_, seed=81)
    xs, dys = _rand(n, 4, d, h, w_, seed=82), _rand(n, 3, d, h, w_, seed=83)
    add("wgrad3_l", True, lambda: as_list(ops.wgrad3_fused(x3, dy3).dw))
    add("wgrad3_l_deferred", True, lambda: as_list(ops.wgrad3_fused(x3, dy3, deferred=True).dw))
    add("wgrad3_l_xc4", True, lambda: as_list(ops.wgrad3_fused(xs, dy3, x_c4=True, dw_cin=4).dw))
    add("wgrad3_l_dyc4", True, lambda: as_list(ops.wgrad3_fused(x3, dys, dy_c4=True, dw_cout=3).dw))

    # ---- ru_criterion_sums, ru_zscore_stats, ru_case_stats at the smallest two-tile shapes of tests/test_scalar_passes_host.py: 2 x 3 classes at V = 8192 + 1,
    # 4 channels at V = 16384 + 1, a 40 x 40 x 21 box.  The criterion refuses a short workspace with RU_ENOMEM; the two statistics entries refuse it too, but as a bad
    # argument (RU_EINVAL, "... workspace too small"), so they have no short case
    from brats2019_amd import _lib as L
    pc, gc = torch.sigmoid(_rand(2, 3, 8193, seed=130, scale=3.0)), (_rand(2, 3, 8193, seed=131) > 0.5).float()
    add("criterion_sums", True, lambda: as_list(ops.criterion_sums(pc, gc)))
    xz = _rand(4, 16385, seed=132, scale=100.0)

    def zscore():
        lib = L.load()
        stats = torch.empty((4, 3), dtype=torch.float64, device=xz.device)
        ws = L.workspace(lib.ru_zscore_workspace_bytes(4, 16385), xz.device)
        L.check(lib.ru_zscore_stats(L.f32(xz), L.ptr(stats), 4, 16385, L.ptr(ws), ws.numel(), L.stream()), "ru_zscore_stats")
        return [stats]
    add("zscore_stats", False, zscore)                  # (brats2019_amd.dataloader.zscore_stats returns host numbers: the entry is called as it calls it)
    xb = _rand(4, 42, 41, 23, seed=133, scale=100.0)
    add("case_stats", False, lambda: as_list(ops.case_stats(xb, (1, 1, 2), (40, 40, 21))))

    # ---- ru_crit_moments at 2 x 3 classes, V = 8192 + 1 (two tiles, the one-by-one form), with and without the log moments.  Like the two statistics entries it
    # refuses a short workspace as a bad argument (RU_EINVAL, "ru_crit_moments: workspace too small"), not with RU_ENOMEM: no short case
    add("crit_moments_logs", False, lambda: as_list(ops.crit_moments(pc, gc)))
    add("crit_moments_no_logs", False, lambda: as_list(ops.crit_moments(pc, gc, mask=L.CRIT_MASK_ALL & ~L.CRIT_MASK_LOGS)))

    # ---- ru_intensity_augment through dataloader.intensity_augment: 4 channels at 3 x 3 x 911 (V = 8192 + 7: two partials per statistic), every carve of the
    # workspace in use -- both blur intermediates, the low-res tables, the partials and statistics of all three levels.  It refuses a short workspace as a bad
    # argument (RU_EINVAL, "ru_intensity_augment: workspace too small"), not with RU_ENOMEM: no short case
    from brats2019_amd import dataloader as DL
    xi = _rand(4, 3, 3, 911, seed=140)
    qi = [dict(blur_sigma=1.0, lowres_zoom=0.63, noise_variance=0.1, noise_seed=4, brightness=1.25, contrast=0.75, gamma=1.5, gamma_invert=True, gamma_retain_stats=True),
          dict(blur_sigma=2.0), {}, dict(lowres_zoom=0.5, gamma=0.7)]
    add("intensity_augment", False, lambda: as_list(DL.intensity_augment(xi, qi)))
    return out
