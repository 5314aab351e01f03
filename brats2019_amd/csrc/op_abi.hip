// op_abi.hip -- the op-level C-ABI of libresunet_hip.so: the entry points that drive ONE kernel (or one small chain) at a time, for the tests, the tools and
// bench.py's roofline probe.  No kernels of its own but gn_scale_shift_kernel; everything else is a launcher of another unit.
//
// Every entry that takes a workspace is a wrapper and a walk.  The extern "C" wrapper checks pointers and arguments, puts an Arena (arena.hpp) over
// (ws, ws_bytes), calls the walk and turns a failed arena into RU_ENOMEM.  The static walk allocates with A.alloc only and launches and packs through
// RU_ARENA_RUN only, so it runs with null tensor pointers on a host without a device -- and each ru_*_workspace_bytes query IS that walk on a dry arena
// (plus kSlack): no formula restates a carve.  A query that serves several walks returns the largest of them.
#include "ru_common.h"
#include "arena.hpp"

#include <math.h>

namespace ru {

__global__ void gn_scale_shift_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                                      const float* __restrict__ rstd, float* __restrict__ scale, float* __restrict__ shift, int N, int C, int G) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, c = i % C, g = c / (C / G);
    const float a = gamma[c] * rstd[n * G + g];
    scale[i] = a;
    shift[i] = beta[c] - mean[n * G + g] * a;
}
static int gn_scale_shift_launch(const float* gamma, const float* beta, const float* mean, const float* rstd, float* scale, float* shift, int N, int C, int G, hipStream_t s) {
    hipLaunchKernelGGL(gn_scale_shift_kernel, dim3(cdiv(N * C, 256)), dim3(256), 0, s, gamma, beta, mean, rstd, scale, shift, N, C, G);
    RU_CHECK_LAUNCH("gn_scale_shift_kernel");
    return RU_OK;
}

}  // namespace ru

using namespace ru;

constexpr size_t kSlack = 4096;            // what every query adds to its walk

static Arena arena_over(void* ws, size_t ws_bytes) {
    Arena A;
    A.dry = false; A.base = (char*)ws; A.cap = ws ? ws_bytes : 0;
    return A;
}
static int walk_result(const Arena& A, int rc) {
    if (rc) return rc;
    if (A.failed) { set_error("workspace too small"); return RU_ENOMEM; }
    return RU_OK;
}
// bytes the walk takes: walk(A) on a dry arena (its return value -- a shape the entry refuses -- does not matter to the size)
template <class F>
static size_t dry_need(F&& walk) {
    Arena A;
    (void)walk(A);
    return A.need();
}

// ====================================================================== NCDHW convolutions, k = 1 / 2 / 3
// pack one 3x3x3 weight for `precision` into the workspace and fill the weight fields of `a`
static int prep_conv3_weights(Conv3Args& a, const float* w, int Cin_f, int Cout_f, int mode, int precision, int W, Arena& A, hipStream_t s) {
    const int cin_conv = mode == 0 ? Cin_f : Cout_f, cout_conv = mode == 0 ? Cout_f : Cin_f;
    a.mode = precision;
    if (conv3_effective_mode(precision, W) == RU_PREC_BF16X3) {
        void* wf = A.alloc(conv3_sb_frag_bytes(cin_conv, cout_conv) / 4 + 64);
        unsigned wforms = 0;
        RU_ARENA_RUN(conv3_sb_pack_weights(w, wf, Cin_f, Cout_f, mode, s, PACK_ALL, &wforms));
        conv3_set_pack(a, wf, wforms);
        return RU_OK;
    }
    float* wp = A.alloc(conv3_packed_floats(cin_conv, cout_conv));
    a.wp = wp;
    RU_ARENA_RUN(conv3_pack_weights(w, wp, Cin_f, Cout_f, mode, s));
    return RU_OK;
}

static int conv3d_fwd_walk(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int k, int precision,
                           Arena& A, hipStream_t s) {
    if (k == 3) {
        Conv3Args a{};
        int rc = prep_conv3_weights(a, w, Cin, Cout, 0, precision, W, A, s);
        if (rc) return rc;
        a.x = x; a.bias = bias; a.y = y; a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
        RU_ARENA_RUN(conv3_launch(a, switches_from_env(), s));
    } else if (k == 1) {
        float* wT = A.alloc((size_t)Cin * Cout);
        RU_ARENA_RUN(transpose_launch(w, wT, Cout, Cin, s));
        Conv1Args a{};
        a.x0 = x; a.C0 = Cin; a.wT = wT; a.ldw = Cout; a.y = y; a.out_slope = 1.f; a.N = N; a.Cout = Cout; a.V = (size_t)D * H * W;
        RU_ARENA_RUN(conv1_launch(a, s));
    } else if (k == 2) {
        const size_t Vo = (size_t)(D / 2) * (H / 2) * (W / 2);
        float* xs = A.alloc((size_t)N * 8 * Cin * Vo);
        float* wT = A.alloc((size_t)8 * Cin * Cout);
        RU_ARENA_RUN(s2d_launch(x, xs, N, Cin, D, H, W, s));
        RU_ARENA_RUN(transpose_launch(w, wT, Cout, 8 * Cin, s));
        Conv1Args a{};
        a.x0 = xs; a.C0 = 8 * Cin; a.wT = wT; a.ldw = Cout; a.y = y; a.out_slope = 1.f; a.N = N; a.Cout = Cout; a.V = Vo;
        RU_ARENA_RUN(conv1_launch(a, s));
    }
    return RU_OK;
}

static int conv3d_bwd_data_walk(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int D, int H, int W, int k, int precision,
                                Arena& A, hipStream_t s) {
    if (k == 3) {
        Conv3Args a{};
        int rc = prep_conv3_weights(a, w, Cin, Cout, 1, precision, W, A, s);
        if (rc) return rc;
        a.x = dy; a.y = dx; a.N = N; a.Cin = Cout; a.Cout = Cin; a.D = D; a.H = H; a.W = W;
        RU_ARENA_RUN(conv3_launch(a, switches_from_env(), s));
    } else if (k == 1) {
        Conv1Args a{};
        a.x0 = dy; a.C0 = Cout; a.wT = w; a.ldw = Cin; a.y = dx; a.out_slope = 1.f; a.N = N; a.Cout = Cin; a.V = (size_t)D * H * W;
        RU_ARENA_RUN(conv1_launch(a, s));
    } else if (k == 2) {
        const size_t Vo = (size_t)(D / 2) * (H / 2) * (W / 2);
        float* t = A.alloc((size_t)N * 8 * Cin * Vo);
        Conv1Args a{};
        a.x0 = dy; a.C0 = Cout; a.wT = w; a.ldw = 8 * Cin; a.y = t; a.out_slope = 1.f; a.N = N; a.Cout = 8 * Cin; a.V = Vo;
        RU_ARENA_RUN(conv1_launch(a, s));
        RU_ARENA_RUN(d2s_launch(t, dx, N, Cin, D, H, W, s));
    }
    return RU_OK;
}

// with_db: the bias gradient is wanted too (k = 3; its own flag so that a dry walk can ask for it without a pointer)
static int conv3d_bwd_weight_walk(const float* x, const float* dy, float* dw, float* db, bool with_db, int N, int Cin, int Cout, int D, int H, int W, int k,
                                  int precision, Arena& A, hipStream_t s) {
    if (k == 3) {
        Wgrad3Args a{};
        a.x = x; a.dy = dy; a.dw = dw; a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W; a.mode = precision;
        a.ws_bytes = wgrad3_workspace_bytes(N, Cin, Cout, D, H, W);
        a.ws = A.alloc(a.ws_bytes / 4);
        RU_ARENA_RUN(wgrad3_launch(a, s));
        if (with_db) {
            const size_t b = bias_grad_workspace_bytes(N, Cout, (size_t)D * H * W);
            float* p = A.alloc(b / 4 + 1);
            RU_ARENA_RUN(bias_grad_launch(dy, db, N, Cout, (size_t)D * H * W, p, b, s));
        }
    } else if (k == 1) {
        Wgrad1Args a{};
        a.x = x; a.dy = dy; a.dw = dw; a.ldw = Cin; a.N = N; a.Cin = Cin; a.Cout = Cout; a.V = (size_t)D * H * W;
        a.ws_bytes = wgrad1_workspace_bytes(N, Cin, Cout, a.V);
        a.ws = A.alloc(a.ws_bytes / 4);
        RU_ARENA_RUN(wgrad1_launch(a, s));
    } else if (k == 2) {
        const size_t Vo = (size_t)(D / 2) * (H / 2) * (W / 2);
        float* xs = A.alloc((size_t)N * 8 * Cin * Vo);
        RU_ARENA_RUN(s2d_launch(x, xs, N, Cin, D, H, W, s));
        Wgrad1Args a{};
        a.x = xs; a.dy = dy; a.dw = dw; a.ldw = 8 * Cin; a.N = N; a.Cin = 8 * Cin; a.Cout = Cout; a.V = Vo;
        a.ws_bytes = wgrad1_workspace_bytes(N, 8 * Cin, Cout, Vo);
        a.ws = A.alloc(a.ws_bytes / 4);
        RU_ARENA_RUN(wgrad1_launch(a, s));
    }
    return RU_OK;
}

// what ru_conv3d_fwd / _bwd_data / _bwd_weight (and their _p forms) share: precision, kernel size, and what only k = 3 / even extents take
static int conv3d_check(const char* who, int precision, int k, bool has_bias, int D, int H, int W) {
    RU_REQUIRE(precision == RU_PREC_F32 || precision == RU_PREC_BF16X3, "%s: bad precision", who);
    RU_REQUIRE(k == 1 || k == 2 || k == 3, "%s: unsupported kernel size %d", who, k);
    RU_REQUIRE(k == 3 || !has_bias, "%s: bias only supported for k=3 (model.py:348)", who);
    RU_REQUIRE(k != 2 || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), "%s: k=2 needs even extents", who);
    return RU_OK;
}

extern "C" int ru_conv3d_fwd_p(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int k,
                               int precision, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && w && y, "ru_conv3d_fwd: null argument");
    int rc = conv3d_check("ru_conv3d_fwd", precision, k, bias != nullptr, D, H, W);
    if (rc) return rc;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3d_fwd_walk(x, w, bias, y, N, Cin, Cout, D, H, W, k, precision, A, (hipStream_t)stream));
}
extern "C" int ru_conv3d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int k,
                             void* ws, size_t ws_bytes, ru_stream_t stream) {
    return ru_conv3d_fwd_p(x, w, bias, y, N, Cin, Cout, D, H, W, k, RU_PREC_F32, ws, ws_bytes, stream);
}

extern "C" int ru_conv3d_bwd_data_p(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int D, int H, int W, int k,
                                    int precision, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(dy && w && dx, "ru_conv3d_bwd_data: null argument");
    int rc = conv3d_check("ru_conv3d_bwd_data", precision, k, false, D, H, W);
    if (rc) return rc;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3d_bwd_data_walk(dy, w, dx, N, Cin, Cout, D, H, W, k, precision, A, (hipStream_t)stream));
}
extern "C" int ru_conv3d_bwd_data(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int D, int H, int W, int k,
                                  void* ws, size_t ws_bytes, ru_stream_t stream) {
    return ru_conv3d_bwd_data_p(dy, w, dx, N, Cin, Cout, D, H, W, k, RU_PREC_F32, ws, ws_bytes, stream);
}

extern "C" int ru_conv3d_bwd_weight_p(const float* x, const float* dy, float* dw, float* db, int N, int Cin, int Cout, int D, int H, int W, int k,
                                      int precision, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && dy && dw, "ru_conv3d_bwd_weight: null argument");
    int rc = conv3d_check("ru_conv3d_bwd_weight", precision, k, db != nullptr, D, H, W);
    if (rc) return rc;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3d_bwd_weight_walk(x, dy, dw, db, db != nullptr, N, Cin, Cout, D, H, W, k, precision, A, (hipStream_t)stream));
}
extern "C" int ru_conv3d_bwd_weight(const float* x, const float* dy, float* dw, float* db, int N, int Cin, int Cout, int D, int H, int W, int k,
                                    void* ws, size_t ws_bytes, ru_stream_t stream) {
    return ru_conv3d_bwd_weight_p(x, dy, dw, db, N, Cin, Cout, D, H, W, k, RU_PREC_F32, ws, ws_bytes, stream);
}

// The split-K form of the exact-f32 NCDHW 3x3x3 forward, as the engine's small f32 shapes run it (conv3_launch_splitk: partial tensors, the launch with
// Conv3Args::ksplit, sum_partials_launch).  ksplit = 0: the factor conv3_f32_ksplit gives the shape; 1 (given or chosen): the plain launch.  The launcher refuses a
// factor that does not divide the input-channel chunks and a bias beside a split.
static int conv3d_fwd_splitk_walk(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int ksplit,
                                  Arena& A, hipStream_t s) {
    Conv3Args a{};
    int rc = prep_conv3_weights(a, w, Cin, Cout, 0, RU_PREC_F32, W, A, s);
    if (rc) return rc;
    a.x = x; a.bias = bias; a.y = y; a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    float* part = A.alloc(conv3_splitk_part_floats(N, Cin, Cout, D, H, W, ksplit));
    RU_ARENA_RUN(conv3_launch_splitk(a, part, ksplit, switches_from_env(), s));
    return RU_OK;
}
extern "C" size_t ru_conv3d_fwd_splitk_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int ksplit) {
    return kSlack + dry_need([&](Arena& A) { return conv3d_fwd_splitk_walk(nullptr, nullptr, nullptr, nullptr, N, Cin, Cout, D, H, W, ksplit, A, nullptr); });
}
extern "C" int ru_conv3d_fwd_splitk(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int ksplit,
                                    void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && w && y, "ru_conv3d_fwd_splitk: null argument");
    RU_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0 && ksplit >= 0 && ksplit <= 64, "ru_conv3d_fwd_splitk: bad shape or split factor");
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3d_fwd_splitk_walk(x, w, bias, y, N, Cin, Cout, D, H, W, ksplit, A, (hipStream_t)stream));
}

// ---------------------------------------------------------------------- what a launch of the NCDHW family would choose: host-only queries (no launch, no workspace)
// of the functions the launchers themselves switch on
extern "C" int ru_conv3_f32_inst(int N, int Cin, int Cout, int D, int H, int W) {
    RU_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "ru_conv3_f32_inst: bad shape");
    return conv3_f32_inst(N, Cin, Cout, D, H, W);
}
extern "C" int ru_wgrad3_inst(int N, int Cin, int Cout, int D, int H, int W, int precision, int flags, int* out7) {
    RU_REQUIRE(out7 && N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "ru_wgrad3_inst: bad argument");
    Wgrad3Args a{};
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W; a.mode = precision; a.x_c16 = flags & 1; a.dy_c16 = (flags >> 1) & 1;
    const W3Inst i = wgrad3_inst(a);
    out7[0] = i.kernel; out7[1] = i.ot; out7[2] = i.ct; out7[3] = i.x16; out7[4] = i.dy16; out7[5] = i.nbx; out7[6] = i.ntile;
    return RU_OK;
}
extern "C" int ru_conv1_inst(int N, int Cin, int Cout, size_t V) {
    RU_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && V > 0, "ru_conv1_inst: bad shape");
    Conv1Args a{};
    a.N = N; a.C0 = Cin; a.Cout = Cout; a.V = V;
    return conv1_inst(a);
}
extern "C" int ru_wgrad1_inst(int N, int Cin, int Cout, size_t V, int* out3) {
    RU_REQUIRE(out3 && N > 0 && Cin > 0 && Cout > 0 && V > 0, "ru_wgrad1_inst: bad argument");
    Wgrad1Args a{};
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.V = V;
    out3[0] = wgrad1_inst(a);
    wgrad1_walk(a, &out3[1], &out3[2]);
    return RU_OK;
}

// ====================================================================== GroupNorm
static int groupnorm_fwd_walk(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean, float* rstd,
                              int N, int C, size_t V, int G, float eps, float slope, Arena& A, hipStream_t s) {
    const int nblk = gn_stats_tiles(V);
    float* part = A.alloc((size_t)N * C * nblk * 2);
    float* scale = A.alloc((size_t)N * C);
    float* shift = A.alloc((size_t)N * C);
    RU_ARENA_RUN(gn_stats_launch(x, part, N, C, V, s));
    RU_ARENA_RUN(gn_finalize_launch(part, nblk, gamma, beta, mean, rstd, scale, shift, N, C, V, G, eps, s, nullptr, true));
    RU_ARENA_RUN(gn_apply_launch(x, scale, shift, residual, y, N, C, V, slope, s));
    return RU_OK;
}
static int groupnorm_bwd_walk(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, const float* dy,
                              float* dx, float* dgamma, float* dbeta, int N, int C, size_t V, int G, float slope, Arena& A, hipStream_t s) {
    const int nblk = gn_bwd_tiles(V);
    float* part = A.alloc((size_t)N * C * nblk * 2);
    float* scale = A.alloc((size_t)N * C);
    float* shift = A.alloc((size_t)N * C);
    float* coef = A.alloc((size_t)N * C * 3);
    RU_ARENA_RUN(gn_scale_shift_launch(gamma, beta, mean, rstd, scale, shift, N, C, G, s));
    RU_ARENA_RUN(gn_bwd_reduce_launch(x, dy, scale, shift, mean, rstd, slope, part, N, C, V, G, s));
    RU_ARENA_RUN(gn_bwd_finalize_launch(part, nblk, gamma, mean, rstd, coef, dgamma, dbeta, N, C, V, G, s));
    RU_ARENA_RUN(gn_bwd_apply_launch(x, dy, scale, shift, coef, slope, dx, N, C, V, s));
    return RU_OK;
}

extern "C" size_t ru_groupnorm_workspace_bytes(int N, int C, size_t V) {
    const size_t f = dry_need([&](Arena& A) { return groupnorm_fwd_walk(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, C, V, 8, 0.f, 1.f, A, nullptr); });
    const size_t b = dry_need([&](Arena& A) { return groupnorm_bwd_walk(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, C, V, 8, 1.f, A, nullptr); });
    return kSlack + (f > b ? f : b);
}
extern "C" int ru_groupnorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean, float* rstd,
                                int N, int C, size_t V, int G, float eps, float slope, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && gamma && beta && y && mean && rstd, "ru_groupnorm_fwd: null argument");
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, groupnorm_fwd_walk(x, gamma, beta, residual, y, mean, rstd, N, C, V, G, eps, slope, A, (hipStream_t)stream));
}
extern "C" int ru_groupnorm_bwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, const float* dy,
                                float* dx, float* dgamma, float* dbeta, int N, int C, size_t V, int G, float slope,
                                void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && gamma && beta && mean && rstd && dy && dx, "ru_groupnorm_bwd: null argument");
    RU_REQUIRE(C % G == 0, "ru_groupnorm_bwd: C %% G != 0");
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, groupnorm_bwd_walk(x, gamma, beta, mean, rstd, dy, dx, dgamma, dbeta, N, C, V, G, slope, A, (hipStream_t)stream));
}

extern "C" int ru_leaky_relu_fwd(const float* x, float* y, size_t n, float slope, ru_stream_t stream) { return lrelu_fwd_launch(x, y, n, slope, (hipStream_t)stream); }
extern "C" int ru_leaky_relu_bwd(const float* y, const float* dy, float* dx, size_t n, float slope, ru_stream_t stream) { return lrelu_bwd_launch(y, dy, dx, n, slope, (hipStream_t)stream); }
extern "C" int ru_upsample2x_trilinear_fwd(const float* x, float* y, int N, int C, int D, int H, int W, ru_stream_t stream) { return up2_fwd_launch(x, y, N, C, D, H, W, (hipStream_t)stream); }
extern "C" int ru_upsample2x_trilinear_bwd(const float* dy, float* dx, int N, int C, int D, int H, int W, ru_stream_t stream) { return up2_bwd_launch(dy, dx, N, C, D, H, W, (hipStream_t)stream); }
extern "C" int ru_sigmoid_fwd(const float* x, float* y, size_t n, ru_stream_t stream) { return sigmoid_launch(x, y, n, (hipStream_t)stream); }

extern "C" size_t ru_criterion_workspace_bytes(int N, int C, size_t V) { return 4096 + (size_t)N * C * crit_tiles(V) * 3 * sizeof(float); }
extern "C" int ru_criterion_sums(const float* p, const float* g, double* sums, int N, int C, size_t V, float bg_weight, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(p && g && sums, "ru_criterion_sums: null argument");
    return crit_sums_launch(p, g, sums, N, C, V, bg_weight, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int ru_criterion_grad(const float* p, const float* g, const double* sums, double count, float w_dice, float w_bce, float bg_weight,
                                 float priority, float* dp, int N, int C, size_t V, ru_stream_t stream) {
    RU_REQUIRE(p && g && sums && dp && count > 0, "ru_criterion_grad: bad argument");
    return crit_grad_launch(p, g, sums, count, w_dice, w_bce, bg_weight, priority, dp, N, C, V, (hipStream_t)stream);
}
extern "C" int ru_criterion_value(const double* sums_host, int C, double count, double priority, double* dice, double* bce) {
    RU_REQUIRE(sums_host && C > 0 && count > 0, "ru_criterion_value: bad argument");
    double acc = 0.0;
    for (int c = 0; c < C; ++c) acc += 2.0 * (sums_host[c] + 1e-6) / (sums_host[C + c] + 2e-6);   // loss.py:114-117
    if (dice) *dice = priority * (1.0 - acc / C);                                                  // loss.py:122
    if (bce) *bce = -sums_host[2 * C] / count;                                                     // loss.py:79
    return RU_OK;
}
extern "C" int ru_criterion_value_device(const double* sums, int C, double count, double priority, double w_dice, double w_bce, double* out3,
                                         ru_stream_t stream) {
    RU_REQUIRE(sums && out3 && C > 0 && C <= 64 && count > 0, "ru_criterion_value_device: bad argument");
    return crit_value_launch(sums, C, count, priority, w_dice, w_bce, out3, (hipStream_t)stream);
}
extern "C" int ru_adam_amsgrad_step(float* w, const float* g, float* m, float* v, float* vmax, size_t n, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int step, ru_stream_t stream) {
    RU_REQUIRE(w && g && m && v && vmax, "ru_adam_amsgrad_step: null argument");
    return adam_launch(w, g, m, v, vmax, n, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

extern "C" int ru_adam_step(float* w, const float* g, float* m, float* v, float* vmax_or_null, size_t n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int step, ru_stream_t stream) {
    RU_REQUIRE(w && g && m && v, "ru_adam_step: null argument");
    return adam_launch(w, g, m, v, vmax_or_null, n, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

// ---------------------------------------------------------------- inference post-processing
extern "C" int ru_tta_merge(const float* probs, int K, unsigned flips, float* mean_out, unsigned char* mask, unsigned long long* counts,
                            int C, int D, int H, int W, ru_stream_t stream) {
    RU_REQUIRE(probs && mask && counts, "ru_tta_merge: null argument");
    RU_REQUIRE(K >= 1 && K <= 8 && C >= 1, "tta_merge: 1..8 predictions");
    const int lo[3] = {0, 0, 0}, size[3] = {D, H, W};                   // the box covering the whole volume
    return merge_launch("ru_tta_merge", false, probs, K, flips, nullptr, nullptr, 1, 1, 0, mean_out, mask, counts, nullptr, C, D, H, W, lo, size, (hipStream_t)stream);
}
extern "C" int ru_compose_labels(const unsigned char* mask, const unsigned long long* counts, unsigned long long et_min, unsigned char* labels,
                                 size_t V, ru_stream_t stream) {
    RU_REQUIRE(mask && counts && labels, "ru_compose_labels: null argument");
    return compose_labels_launch(mask, counts, et_min, labels, V, (hipStream_t)stream);
}

extern "C" int ru_dice_accumulate(const unsigned long long* counts, double* acc, int N, int C, int nacc, ru_stream_t stream) {
    return dice_accumulate_launch(counts, acc, N, C, nacc, (hipStream_t)stream);
}
extern "C" int ru_dice_counts(const float* p, const float* g, unsigned long long* counts, int N, int C, size_t V, ru_stream_t stream) {
    RU_REQUIRE(p && g && counts && N > 0 && C > 0, "ru_dice_counts: bad argument");
    return dice_counts_launch(p, g, counts, N * C, V, (hipStream_t)stream);
}

// ====================================================================== C16 layout hooks (tests / probes)
extern "C" int ru_layout_convert(const float* src, float* dst, int N, int C, size_t V, int to_c16, ru_stream_t stream) {
    RU_REQUIRE(src && dst && N > 0, "ru_layout_convert: bad argument");
    return layout_convert_launch(src, dst, N, C, V, to_c16, (hipStream_t)stream);
}

extern "C" int ru_upsample2x_trilinear_fwd_l(const float* x, float* y, int N, int C, int D, int H, int W, float out_slope, ru_stream_t stream) {
    RU_REQUIRE(x && y && N > 0 && C > 0 && D > 0 && H > 0 && W > 0, "ru_upsample2x_trilinear_fwd_l: bad argument");
    return up2_fwd16_launch(x, y, N, C, D, H, W, out_slope, (hipStream_t)stream);
}
extern "C" int ru_upsample2x_trilinear_bwd_l(const float* dy, float* dx, int N, int C, int D, int H, int W, ru_stream_t stream) {
    RU_REQUIRE(dy && dx && N > 0 && C > 0 && D > 0 && H > 0 && W > 0, "ru_upsample2x_trilinear_bwd_l: bad argument");
    return up2_bwd16_launch(dy, dx, N, C, D, H, W, (hipStream_t)stream);
}

// ru_fin_desc -> FinTail (what the caller left 0 of nblk / N / C is the launch's own)
static void fill_fin(FinTail& f, const ru_fin_desc& d, unsigned* ticket, int nblk, int N, int C, size_t V) {
    f.ticket = ticket; f.kind = d.kind; f.nblk = d.nblk ? d.nblk : nblk; f.N = d.N ? d.N : N; f.C = d.C ? d.C : C; f.G = d.G; f.V = V; f.eps = d.eps; f.s2_sign = d.s2_sign;
    f.gamma = d.gamma; f.beta = d.beta; f.mean = d.mean; f.rstd = d.rstd; f.scale = d.scale; f.shift = d.shift; f.bst_k = d.bst_k;
    f.coef = d.coef; f.dgamma = d.dgamma; f.dbeta = d.dbeta;
}
static int fin_desc_check(const char* who, const ru_fin_desc& d, int C) {
    RU_REQUIRE(d.kind == 1 || d.kind == 2, "%s: the tail's kind is 1 (statistics) or 2 (GroupNorm-backward sums)", who);
    RU_REQUIRE(d.G > 0 && C % d.G == 0, "%s: the tail needs G groups with C %% G == 0", who);
    RU_REQUIRE(d.gamma && d.mean && d.rstd, "%s: the tail needs gamma, mean and rstd", who);
    RU_REQUIRE(d.kind != 1 || (d.beta && d.scale && d.shift), "%s: a kind-1 tail needs beta, scale and shift", who);
    RU_REQUIRE(d.kind != 2 || d.coef, "%s: a kind-2 tail needs coef", who);
    return RU_OK;
}
// The 3x3x3 family, one launch at a time with every fused operand of Conv3Args (ksplit has its own entry, ru_conv3d_fwd_splitk, held by tests/test_ncdhw_convs.py): a thin filler.  The caller (`who`, for the messages) has put the
// tensors, the shape and the fused operands into `a`; the walk decodes `flags` (resunet_hip.h), packs w and launches.  weight_mode = 1 packs the data-gradient form of
// w = [Cout][Cin][3][3][3] OF THE FORWARD CONVOLUTION (channels swapped, taps mirrored), so that the launch maps x's Cin channels (the forward's outputs) to y's Cout
// channels as the engine's backward does.  ru_conv3d_fwd_l is this walk with weight_mode 0 and no fused operands or reports.  fd (flag bit 8 on a dry walk): the tail
// finalize -- Conv3Args::fin filled as the engine's conv3_gn / fill_bwd_tail fill it, the ticket a word of the workspace, zeroed on the stream (a workspace arrives
// with anything in it).
static int conv3_l_walk(const char* who, Conv3Args a, const float* w, int flags, int weight_mode, size_t stat_floats, int* nblk, int* route, Arena& A, hipStream_t s,
                        const ru_fin_desc* fd = nullptr) {
    const Switches sw = switches_from_env();
    const int N = a.N, Cin = a.Cin, Cout = a.Cout, D = a.D, H = a.H, W = a.W;
    const bool f32 = (flags & 16) != 0;                          // exact-f32 arithmetic on voxel-major tensors (conv3_f32c_kernel)
    void* wf = A.alloc((f32 ? conv3_f32c_frag_bytes(Cin, Cout) : conv3_sb_frag_bytes(Cin, Cout)) / 4 + 64);
    if (flags & 32) a.products = 2;                              // the input is an activation tensor: fp16 + MX-fp8 products where the shape has that kernel (conv3_mx.hpp)
    RU_REQUIRE(!f32 || ((flags & 3) != 0 && !(flags & (4 | 8))), "%s: the exact-f32 form needs a voxel-major side and takes neither the 4-channel copy nor a split-form input", who);
    // flag bit 6: x (float32, voxel-major) is a GRADIENT -- where conv3_mx_kernel<GRAD> takes the shape it is converted to the gradient-operand form of the MX scheme
    // (conv3_mxg_split_launch; in a training step wgrad3_tz<1,0,3,3> writes that form) and convolved with bf16 main + MX cross products; elsewhere the bit is ignored
    const bool gop = (flags & 64) && !f32 && (flags & 3) == 3 && !(flags & (4 | 8)) && !a.bias && conv3_mxg_usable(sw, N, Cin, Cout, D, H, W);
    const int Cin_f = weight_mode ? Cout : Cin, Cout_f = weight_mode ? Cin : Cout;       // w's own extents [Cout_f][Cin_f][27]
    a.mode = f32 ? RU_PREC_F32 : RU_PREC_BF16X3;
    a.in_c16 = flags & 1; a.out_c16 = (flags >> 1) & 1;
    int forms = PACK_ALL | (gop ? PACK_MX_GRAD : 0);             // (the MX fragments of a weight exist in ONE variant: activation or gradient operand)
    // flag bit 7: pack w as a training step does (engine.hip, pack_all) -- the forms the switches launch, and no direct fragments where a forward convolution of
    // this shape and these layouts, without the fused operands of this call, takes a Winograd-z / MX route
    if (flags & 128) {
        Conv3Args fwd{};
        fwd.mode = a.mode; fwd.N = N; fwd.Cin = Cin; fwd.Cout = Cout; fwd.D = D; fwd.H = H; fwd.W = W;
        fwd.in_c16 = a.in_c16; fwd.out_c16 = a.out_c16; fwd.products = a.products;
        forms = sb_pack_forms(sw, weight_mode) | ((weight_mode == 0 && conv3_route_skips_direct(conv3_sb_route(fwd, sw))) ? PACK_SKIP_DIRECT : 0);
    }
    unsigned wforms = 0;
    RU_ARENA_RUN(f32 ? conv3_f32c_pack_weights(w, wf, Cin_f, Cout_f, weight_mode, s) : conv3_sb_pack_weights(w, wf, Cin_f, Cout_f, weight_mode, s, forms, &wforms));
    conv3_set_pack(a, wf, wforms);
    a.in_s16 = (flags >> 3) & 1;                                 // x is voxel-major in SPLIT form (hi / lo bf16 packets, as gn_bwd_apply16 publishes it)
    RU_REQUIRE(!a.in_s16 || a.in_c16, "%s: the split form is a voxel-major layout", who);
    if (gop) {
        const size_t nvox = (size_t)N * D * H * W;
        float* g16 = A.alloc(nvox * 16);
        RU_ARENA_RUN(conv3_mxg_split_launch(a.x, g16, nvox, s));
        a.x = g16; a.in_s16 = 1; a.in_g16 = 1; a.products = 0;
    }
    if (flags & 4) {                                             // x NCDHW with Cin <= 4: 4-channel copy + tap-pair kernel
        RU_REQUIRE(!(flags & 1) && conv3_sb4_usable(N, Cin, Cout, D, H, W), "%s: shape does not fit the 4-channel kernel", who);
        const size_t V = (size_t)D * H * W;
        float* x4 = A.alloc((size_t)N * 4 * V);
        void* wf4 = A.alloc(conv3_sb4_frag_bytes(Cout) / 4 + 64);
        RU_ARENA_RUN(pad_to_c4_launch(a.x, x4, N, Cin, V, s));
        RU_ARENA_RUN(conv3_sb4_pack_weights(w, wf4, Cin_f, Cout_f, weight_mode, s));
        a.x = x4; conv3_set_pack(a, wf4, PACK_HAS_SB4); a.in_c4 = 1;
    }
    unsigned* ticket = (fd || (flags & 256)) ? reinterpret_cast<unsigned*>(A.alloc(64)) : nullptr;
    if (route || nblk || a.stat_partials) {
        const int r = f32 ? conv3_f32c_route(a) : conv3_sb_route(a, sw);
        if (route) *route = r;
        const int nb = f32 ? conv3_f32c_tiles_per_sample(N, Cin, Cout, D, H, W) : conv3_sb_route_nblk(r, N, Cout, D, H, W);     // partials per (sample, channel)
        if (nblk) *nblk = nb;
        RU_REQUIRE(!a.stat_partials || stat_floats >= (size_t)N * Cout * nb * 2, "%s: statistics buffer too small", who);
        if (fd && a.stat_partials && !A.dry && !A.failed) fill_fin(a.fin, *fd, ticket, nb, N, Cout, (size_t)D * H * W);
    }
    if (fd && !fd->keep_ticket) RU_ARENA_RUN(fill_launch(reinterpret_cast<float*>(ticket), 0.f, 1, s));
    RU_ARENA_RUN(f32 ? conv3_launch(a, sw, s) : conv3_sb_launch(a, sw, s));
    return RU_OK;
}
static size_t conv3_l_need(int N, int Cin, int Cout, int D, int H, int W, int flags) {
    Conv3Args a{};
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    return dry_need([&](Arena& A) { return conv3_l_walk("ru_conv3_l", a, nullptr, flags, 0, 0, nullptr, nullptr, A, nullptr); });
}
extern "C" size_t ru_conv3_l_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int flags) { return kSlack + conv3_l_need(N, Cin, Cout, D, H, W, flags); }

extern "C" int ru_conv3_l(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W, int flags, int weight_mode,
                          const float* add, const float* in_scale, const float* in_shift, float in_slope, const float* in_res, float* in_sum_out,
                          int sigmoid, int products, const float* bst_y, const float* bst_k, float bst_slope, float* stat_partials, size_t stat_floats,
                          int* nblk, int* route, void* ws, size_t ws_bytes, ru_stream_t stream, const ru_fin_desc* fin) {
    RU_REQUIRE(x && w && y, "ru_conv3_l: null argument");
    RU_REQUIRE(!fin || stat_partials, "ru_conv3_l: the tail finalizes the statistics of this launch (stat_partials)");
    if (fin) { const int rc = fin_desc_check("ru_conv3_l", *fin, Cout); if (rc) return rc; }
    RU_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "ru_conv3_l: bad shape");
    RU_REQUIRE(weight_mode == 0 || weight_mode == 1, "ru_conv3_l: weight_mode is 0 (forward packing) or 1 (data-gradient packing)");
    Conv3Args a{};
    a.x = x; a.bias = bias; a.y = y; a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    a.add = add; a.in_scale = in_scale; a.in_shift = in_shift; a.in_slope = in_slope; a.in_res = in_res; a.in_sum_out = in_sum_out; a.sigmoid = sigmoid;
    a.products = products; a.bst_y = bst_y; a.bst_k = bst_k; a.bst_slope = bst_slope; a.stat_partials = stat_partials;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3_l_walk("ru_conv3_l", a, w, flags, weight_mode, stat_floats, nblk, route, A, (hipStream_t)stream, fin));
}
extern "C" int ru_conv3d_fwd_l(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D, int H, int W,
                               int flags, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && w && y, "ru_conv3d_fwd_l: null argument");
    Conv3Args a{};
    a.x = x; a.bias = bias; a.y = y; a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3_l_walk("ru_conv3d_fwd_l", a, w, flags, 0, 0, nullptr, nullptr, A, (hipStream_t)stream));
}

static int conv3d_bwd_weight_l_walk(Wgrad3Args a, Arena& A, hipStream_t s) {
    a.ws_bytes = wgrad3_workspace_bytes(a.N, a.Cin, a.Cout, a.D, a.H, a.W);
    a.ws = A.alloc(a.ws_bytes / 4);
    RU_ARENA_RUN(wgrad3_launch(a, s));
    return RU_OK;
}
extern "C" int ru_conv3d_bwd_weight_l(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int D, int H, int W,
                                      int flags, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && dy && dw, "ru_conv3d_bwd_weight_l: null argument");
    Wgrad3Args a{};
    a.x = x; a.dy = dy; a.dw = dw; a.mode = RU_PREC_BF16X3; a.x_c16 = flags & 1; a.dy_c16 = (flags >> 1) & 1;
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv3d_bwd_weight_l_walk(a, A, (hipStream_t)stream));
}

// the largest of the walks this one query serves (resunet_hip.h names them)
extern "C" size_t ru_conv3d_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int k) {
    size_t need = 0;
    auto cover = [&](size_t n) { if (n > need) need = n; };
    for (const int p : {RU_PREC_F32, RU_PREC_BF16X3}) {
        cover(dry_need([&](Arena& A) { return conv3d_fwd_walk(nullptr, nullptr, nullptr, nullptr, N, Cin, Cout, D, H, W, k, p, A, nullptr); }));
        cover(dry_need([&](Arena& A) { return conv3d_bwd_data_walk(nullptr, nullptr, nullptr, N, Cin, Cout, D, H, W, k, p, A, nullptr); }));
        cover(dry_need([&](Arena& A) { return conv3d_bwd_weight_walk(nullptr, nullptr, nullptr, nullptr, true, N, Cin, Cout, D, H, W, k, p, A, nullptr); }));
    }
    if (k == 3) {
        Wgrad3Args a{};
        a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
        cover(dry_need([&](Arena& A) { return conv3d_bwd_weight_l_walk(a, A, nullptr); }));
        for (int flags = 0; flags < 256; ++flags)
            if (!(flags & (4 | 64))) cover(conv3_l_need(N, Cin, Cout, D, H, W, flags));       // bits 2 and 6 take more: ru_conv3_l_workspace_bytes
    }
    return kSlack + need;
}

// ====================================================================== the voxel-major GroupNorm chain, one link at a time (thin: the launchers' own checks refuse)
extern "C" int ru_gn_finalize_l(const float* partials, int nblk, const float* gamma, const float* beta, float* mean, float* rstd, float* scale, float* shift, float* bst_k,
                                int N, int C, size_t V, int G, float eps, int centred, ru_stream_t stream) {
    RU_REQUIRE(partials && gamma && beta && mean && rstd && scale && shift, "ru_gn_finalize_l: null argument");
    RU_REQUIRE(N > 0 && C > 0 && G > 0 && nblk > 0 && V > 0, "ru_gn_finalize_l: bad shape");
    return gn_finalize_launch(partials, nblk, gamma, beta, mean, rstd, scale, shift, N, C, V, G, eps, (hipStream_t)stream, bst_k, centred != 0);
}
extern "C" int ru_gn_apply_l(const float* x, const float* scale, const float* shift, const float* res, const float* res_scale, const float* res_shift, float* y,
                             int N, int C, size_t V, float slope, float res_slope, ru_stream_t stream) {
    RU_REQUIRE(x && scale && shift && y, "ru_gn_apply_l: null argument");
    RU_REQUIRE(N > 0 && C > 0 && V > 0, "ru_gn_apply_l: bad shape");
    return gn_apply16_launch(x, scale, shift, res, y, N, C, V, slope, (hipStream_t)stream, res_scale, res_shift, res_slope);
}
extern "C" int ru_gn_bwd_finalize_l(const float* partials, int nblk, const float* gamma, const float* mean, const float* rstd, float* coef, float* dgamma, float* dbeta,
                                    int N, int C, size_t V, int G, int s2_sign, ru_stream_t stream) {
    RU_REQUIRE(partials && gamma && mean && rstd && coef, "ru_gn_bwd_finalize_l: null argument");
    RU_REQUIRE(N > 0 && C > 0 && G > 0 && nblk > 0 && V > 0, "ru_gn_bwd_finalize_l: bad shape");
    return gn_bwd_finalize_launch(partials, nblk, gamma, mean, rstd, coef, dgamma, dbeta, N, C, V, G, (hipStream_t)stream, s2_sign);
}

// the sequence of the engine's gn_bwd() on the voxel-major flow: reduce (with or without the kind-2 tail), finalize where there is no tail, apply (plain or split)
static int copy_out(float* dst, const float* src, size_t nfloats, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(dst, src, nfloats * sizeof(float), hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? RU_OK : hip_fail(e, "hipMemcpyAsync(ru_gn_bwd_l)");
}
static int gn_bwd_l_walk(const float* x, const float* dact, const float* gamma, const float* scale, const float* shift, const float* mean, const float* rstd, float slope,
                         float* dx, float* dgamma, float* dbeta, float* coef_out, float* partials_out, int N, int C, size_t V, int G, int flags, Arena& A, hipStream_t s) {
    const int nblk = gn_bwd_tiles16(V);
    float* part = A.alloc((size_t)N * C * nblk * 2);
    float* coef = A.alloc((size_t)N * C * 3);
    unsigned* ticket = reinterpret_cast<unsigned*>(A.alloc(64));
    FinTail f{};
    if ((flags & 1) && !A.dry && !A.failed) {
        f.ticket = ticket; f.kind = 2; f.nblk = nblk; f.N = N; f.C = C; f.G = G; f.V = V; f.s2_sign = 0;
        f.gamma = gamma; f.mean = const_cast<float*>(mean); f.rstd = const_cast<float*>(rstd); f.coef = coef; f.dgamma = dgamma; f.dbeta = dbeta;
    }
    if ((flags & 1) && !(flags & 8)) RU_ARENA_RUN(fill_launch(reinterpret_cast<float*>(ticket), 0.f, 1, s));
    RU_ARENA_RUN(gn_bwd_reduce16_launch(x, dact, scale, shift, mean, rstd, slope, part, N, C, V, G, s, &f));
    if (!(flags & 1)) RU_ARENA_RUN(gn_bwd_finalize_launch(part, nblk, gamma, mean, rstd, coef, dgamma, dbeta, N, C, V, G, s, 0));
    if (coef_out) RU_ARENA_RUN(copy_out(coef_out, coef, (size_t)N * C * 3, s));
    if (partials_out) RU_ARENA_RUN(copy_out(partials_out, part, (size_t)N * C * nblk * 2, s));
    if (!(flags & 4)) RU_ARENA_RUN(gn_bwd_apply16_launch(x, dact, scale, shift, coef, slope, dx, N, C, V, (flags >> 1) & 1, s));
    return RU_OK;
}
extern "C" int ru_gn_bwd_l_nblk(size_t V) { return gn_bwd_tiles16(V); }
extern "C" size_t ru_gn_bwd_l_workspace_bytes(int N, int C, size_t V) {
    return kSlack + dry_need([&](Arena& A) { return gn_bwd_l_walk(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                  N, C, V, 8, 0, A, nullptr); });
}
extern "C" int ru_gn_bwd_l(const float* x, const float* dact, const float* gamma, const float* scale, const float* shift, const float* mean, const float* rstd, float slope,
                           float* dx, float* dgamma, float* dbeta, float* coef_out, float* partials_out, int N, int C, size_t V, int G, int flags,
                           void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && dact && gamma && scale && shift && mean && rstd && (dx || (flags & 4)), "ru_gn_bwd_l: null argument");
    RU_REQUIRE(N > 0 && C > 0 && G > 0 && V > 0, "ru_gn_bwd_l: bad shape");
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, gn_bwd_l_walk(x, dact, gamma, scale, shift, mean, rstd, slope, dx, dgamma, dbeta, coef_out, partials_out, N, C, V, G, flags, A, (hipStream_t)stream));
}

// ====================================================================== the head of the backward pass, one route of the engine's head_bwd at a time
// route 0: head_grad_c4_launch (and sigmoid_bwd_launch where dlog is wanted, as the engine adds it for a wide first level); 1: head_grad_c4_crit_launch
// (`cg` is the criterion, dp is not read); 2: sigmoid_bwd_launch then bias_grad_launch (any C and V; d4 is not written).  The launchers' own checks refuse.
static int head_grad_l_walk(const float* p, const float* dp, const CritGradArgs& cg, float* d4, float* db, float* dlog, int N, int C, size_t V, int route,
                            Arena& A, hipStream_t s) {
    const size_t wsb = bias_grad_workspace_bytes(N, C, V);
    float* wsp = A.alloc(wsb / sizeof(float) + 1);
    if (route == 1) {
        RU_ARENA_RUN(head_grad_c4_crit_launch(p, cg, d4, db, N, C, V, wsp, wsb, s));
    } else if (route == 0) {
        RU_ARENA_RUN(head_grad_c4_launch(p, dp, d4, db, N, C, V, wsp, wsb, s));
        if (dlog) RU_ARENA_RUN(sigmoid_bwd_launch(p, dp, dlog, (size_t)N * C * V, s));
    } else {
        RU_ARENA_RUN(sigmoid_bwd_launch(p, dp, dlog, (size_t)N * C * V, s));
        RU_ARENA_RUN(bias_grad_launch(dlog, db, N, C, V, wsp, wsb, s));
    }
    return RU_OK;
}
extern "C" size_t ru_head_grad_l_workspace_bytes(int N, int C, size_t V, int route) {
    return kSlack + dry_need([&](Arena& A) { return head_grad_l_walk(nullptr, nullptr, CritGradArgs{}, nullptr, nullptr, nullptr, N, C, V, route, A, nullptr); });
}
extern "C" int ru_head_grad_l(const float* p, const float* dp, const float* target, const double* sums, double count, float w_dice, float w_bce, float bg_weight,
                              float priority, float* d4, float* db, float* dlog, int N, int C, size_t V, int route, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(route >= 0 && route <= 2, "ru_head_grad_l: route is 0 (4-channel pass), 1 (4-channel pass with the criterion) or 2 (sigmoid backward, then bias gradient)");
    RU_REQUIRE(p && db && (route == 1 || dp) && (route == 2 ? dlog != nullptr : d4 != nullptr), "ru_head_grad_l: null argument");
    RU_REQUIRE(route != 1 || (!dlog && count > 0), "ru_head_grad_l: the criterion route writes no dlog and needs a positive count");
    RU_REQUIRE(N > 0 && C > 0 && V > 0, "ru_head_grad_l: bad shape");
    const CritGradArgs cg{target, sums, count, w_dice, w_bce, bg_weight, priority};
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, head_grad_l_walk(p, dp, cg, d4, db, dlog, N, C, V, route, A, (hipStream_t)stream));
}

// The voxel-major pointwise family, one launch at a time: thin fillers of Conv1Args / Wgrad1Args (no kernels, no arithmetic of their own).
static int conv1_l_walk(Conv1Args a, const float* w, size_t stat_floats, int* nblk, int* inst, Arena& A, hipStream_t s) {
    if (a.s2d) {
        // w is the reference's [Cconv_out][Cconv_in][2][2][2]; the engine's pack gives the gather its [Cout][tap*Cin + c] and the scatter its [tap*Cin + c][C0]
        const int co = a.s2d == 1 ? a.Cout : a.C0, ci = (a.s2d == 1 ? a.C0 : a.Cout) / 8;
        float* wd = A.alloc((size_t)8 * ci * co);
        float* wdT = A.alloc((size_t)8 * ci * co);
        RU_ARENA_RUN(pack_down16_launch(w, wd, wdT, co, ci, s));
        a.wT = a.s2d == 1 ? wd : wdT;
        a.ldw = a.C0;
    }
    if (inst) *inst = conv1_16_choose(a).packed();
    if (nblk) *nblk = 0;
    if (a.bst_y) {
        const int nb = conv1_16_bst_nblk(a);             // 0: no fused form -- conv1_16_launch refuses below, with its own message
        RU_REQUIRE(nb == 0 || (a.stat_partials && stat_floats >= (size_t)a.N * (a.s2d == 2 ? a.Cout / 8 : a.Cout) * nb * 2), "ru_conv1_l: statistics buffer too small");
        if (nblk) *nblk = nb;
    }
    RU_ARENA_RUN(conv1_16_launch(a, s));
    return RU_OK;
}
extern "C" size_t ru_conv1_l_workspace_bytes(int C0, int Cout, int s2d) {
    Conv1Args a{};
    a.C0 = C0; a.Cout = Cout; a.s2d = s2d;
    return kSlack + dry_need([&](Arena& A) { return conv1_l_walk(a, nullptr, 0, nullptr, nullptr, A, nullptr); });
}
extern "C" int ru_conv1_l(const float* x0, int C0, const float* x1, int C1, const float* w, int ldw, float* y, float* y1, int Cout0,
                          const float* add, float out_slope, const float* mask, float mask_slope, int N, int Cout, size_t V,
                          int s2d, int Dc, int Hc, int Wc, const float* bst_y, const float* bst_k, float bst_slope,
                          float* stat_partials, size_t stat_floats, int* nblk, int* inst, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x0 && w && y, "ru_conv1_l: null argument");
    RU_REQUIRE(s2d >= 0 && s2d <= 2, "ru_conv1_l: s2d is 0 (plain), 1 (gather) or 2 (scatter)");
    RU_REQUIRE(!s2d || (C0 > 0 && Cout > 0 && (s2d == 1 ? C0 : Cout) % 8 == 0), "ru_conv1_l: stride-2 modes need 8 x channels on the gathered side");
    Conv1Args a{};
    a.x0 = x0; a.C0 = C0; a.x1 = x1; a.C1 = C1; a.wT = w; a.ldw = ldw; a.y = y; a.add = add; a.out_slope = out_slope;
    a.N = N; a.Cout = Cout; a.V = V; a.s2d = s2d; a.Dc = Dc; a.Hc = Hc; a.Wc = Wc; a.mask = mask; a.mask_slope = mask_slope;
    a.y1 = y1; a.Cout0 = Cout0; a.bst_y = bst_y; a.bst_k = bst_k; a.bst_slope = bst_slope; a.stat_partials = stat_partials;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, conv1_l_walk(a, w, stat_floats, nblk, inst, A, (hipStream_t)stream));
}

static int wgrad1_l_walk(Wgrad1Args a, int* inst, Arena& A, hipStream_t s) {
    a.ws_bytes = wgrad1_workspace_bytes(a.N, a.Cin, a.Cout, a.V);
    a.ws = A.alloc(a.ws_bytes / 4);
    if (inst) *inst = wgrad1_inst(a);
    RU_ARENA_RUN(wgrad1_launch(a, s));
    return RU_OK;
}
extern "C" size_t ru_wgrad1_l_workspace_bytes(int N, int Cin, int Cout, size_t V) {
    Wgrad1Args a{};
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.V = V;
    return kSlack + dry_need([&](Arena& A) { return wgrad1_l_walk(a, nullptr, A, nullptr); });
}
extern "C" int ru_wgrad1_l(const float* x, const float* x1, int C0, const float* dy, float* dw, int ldw, int N, int Cin, int Cout, size_t V,
                           int c16, int s2d, int Dc, int Hc, int Wc, int tap_split, const float* dg_w, int dg_ldw, float* dg_y0, float* dg_y1,
                           float dg_mask_slope, int* inst, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && dy && dw, "ru_wgrad1_l: null argument");
    RU_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && V > 0, "ru_wgrad1_l: bad shape");
    Wgrad1Args a{};
    a.x = x; a.x1 = x1; a.C0 = C0; a.dy = dy; a.dw = dw; a.ldw = ldw; a.N = N; a.Cin = Cin; a.Cout = Cout; a.V = V;
    a.c16 = c16; a.s2d = s2d; a.Dc = Dc; a.Hc = Hc; a.Wc = Wc; a.tap_split = tap_split;
    a.dg_w = dg_w; a.dg_ldw = dg_ldw; a.dg_y0 = dg_y0; a.dg_y1 = dg_y1; a.dg_mask_slope = dg_mask_slope;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, wgrad1_l_walk(a, inst, A, (hipStream_t)stream));
}

// The transpose-read 3x3x3 weight gradient, one launch at a time with every operand of Wgrad3Args the engine sets: a thin filler like ru_conv3_l (no kernels,
// no arithmetic of its own).  flags: 1 dy is in split form, 2 x is NCDHW with dw_cin <= 4 channels (4-channel copy made here), 4 dy is NCDHW with dw_cout <= 4
// channels (likewise), 8 swapped, 16 gb_g16, 32 the reduction of the partials is deferred to a list of this call's own and flushed behind the kernel.
static int wgrad3_l_walk(Wgrad3Args a, int flags, int* inst, Arena& A, hipStream_t s) {
    a.ws_bytes = wgrad3_tr_workspace_bytes(a.N, a.Cin, a.Cout, a.D, a.H, a.W);
    a.ws = A.alloc(a.ws_bytes / 4);
    const size_t V = (size_t)a.D * a.H * a.W;
    if (a.x_c4) {                                                // a few-channel side arrives NCDHW and is copied as the engine's stem and head copy it
        float* c4 = A.alloc((size_t)a.N * 4 * V);
        RU_ARENA_RUN(pad_to_c4_launch(a.x, c4, a.N, a.dw_cin, V, s));
        a.x = c4;
    }
    if (a.dy_c4) {
        float* c4 = A.alloc((size_t)a.N * 4 * V);
        RU_ARENA_RUN(pad_to_c4_launch(a.dy, c4, a.N, a.dw_cout, V, s));
        a.dy = c4;
    }
    if (inst) *inst = wgrad3_tr_inst(a);
    WgradRedList own;
    if (flags & 32) a.defer = &own;
    RU_ARENA_RUN(wgrad3_tr_launch(a, s));
    if (flags & 32) RU_ARENA_RUN(wgrad_reduce_flush(own, s));
    return RU_OK;
}
extern "C" size_t ru_wgrad3_l_workspace_bytes(int N, int Cin, int Cout, int D, int H, int W, int flags) {
    Wgrad3Args a{};
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W; a.x_c4 = (flags >> 1) & 1; a.dy_c4 = (flags >> 2) & 1;
    return kSlack + dry_need([&](Arena& A) { return wgrad3_l_walk(a, flags, nullptr, A, nullptr); });
}
extern "C" int ru_wgrad3_l(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int D, int H, int W, int flags, int products,
                           const float* in_scale, const float* in_shift, float in_slope, int dw_cin, int dw_cout,
                           const float* gb_y, const float* gb_d, const float* gb_scale, const float* gb_shift, const float* gb_coef, float gb_slope, float* gb_out,
                           int* inst, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && (dy || gb_y) && dw, "ru_wgrad3_l: null argument");
    RU_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "ru_wgrad3_l: bad shape");
    RU_REQUIRE((!(flags & 2) || (dw_cin > 0 && dw_cin <= 4)) && (!(flags & 4) || (dw_cout > 0 && dw_cout <= 4 && dy)),
               "ru_wgrad3_l: a 4-channel copy holds 1..4 channels (dw_cin / dw_cout)");
    Wgrad3Args a{};
    a.x = x; a.dy = dy ? dy : gb_y; a.dw = dw; a.mode = RU_PREC_BF16X3; a.x_c16 = 1; a.dy_c16 = 1;
    a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
    a.in_scale = in_scale; a.in_shift = in_shift; a.in_slope = in_slope; a.dw_cin = dw_cin; a.dw_cout = dw_cout;
    a.dy_s16 = flags & 1; a.x_c4 = (flags >> 1) & 1; a.dy_c4 = (flags >> 2) & 1; a.swapped = (flags >> 3) & 1; a.gb_g16 = (flags >> 4) & 1; a.products = products;
    a.gb_y = gb_y; a.gb_d = gb_d; a.gb_scale = gb_scale; a.gb_shift = gb_shift; a.gb_coef = gb_coef; a.gb_slope = gb_slope; a.gb_out = gb_out;
    Arena A = arena_over(ws, ws_bytes);
    return walk_result(A, wgrad3_l_walk(a, flags, inst, A, (hipStream_t)stream));
}

// ====================================================================== training input pipeline (dataloader.py)
extern "C" size_t ru_zscore_workspace_bytes(int C, size_t V) { return zscore_workspace_bytes(C, V) + 256; }
extern "C" int ru_zscore_stats(const float* image, double* stats, int C, size_t V, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(image && stats && C > 0 && V > 0, "ru_zscore_stats: bad argument");
    return zscore_stats_launch(image, stats, C, V, ws, ws_bytes, (hipStream_t)stream);
}
static int augment_patch_impl(const float* image, const unsigned char* label, const float* soft, const float* mean, const float* inv_std, int C, int D, int H, int W,
                              const int* crop_lo, const int* patch, const double* scale, int flags, const float* gain, const float* bias,
                              float* data_out, float* target_out, ru_stream_t stream) {
    RU_REQUIRE(image && (label || soft) && mean && inv_std && crop_lo && patch && scale && gain && bias && data_out && target_out, "ru_augment_patch: null argument");
    RU_REQUIRE(C > 0 && C <= RU_AUG_MAXC, "ru_augment_patch: 1..%d channels", RU_AUG_MAXC);
    const int dims[3] = {D, H, W};
    AugmentArgs a{};
    a.image = image; a.label = label; a.soft = soft; a.data = data_out; a.target = target_out; a.C = C; a.D = D; a.H = H; a.W = W; a.flags = flags;
    for (int i = 0; i < 3; ++i) {
        RU_REQUIRE(patch[i] > 0 && crop_lo[i] >= 0 && crop_lo[i] + patch[i] <= dims[i], "ru_augment_patch: the crop must lie inside the volume");
        RU_REQUIRE(scale[i] > 0.0, "ru_augment_patch: scale must be positive");
        // zoom_voxel converts floor(scale * index) to int: the largest source coordinate, scale * (P - 1), has to stay well inside its range
        RU_REQUIRE(isfinite(scale[i]), "ru_augment_patch: scale[%d] is not finite", i);
        RU_REQUIRE(scale[i] * (double)(patch[i] - 1) < 1073741824.0, "ru_augment_patch: scale[%d] * (patch[%d] - 1) = %g reaches 2^30", i, i,
                   scale[i] * (double)(patch[i] - 1));
        a.lo[i] = crop_lo[i]; a.P[i] = patch[i]; a.scale[i] = scale[i];
    }
    for (int c = 0; c < C; ++c) { a.mean[c] = mean[c]; a.istd[c] = inv_std[c]; a.gain[c] = gain[c]; a.bias[c] = bias[c]; }
    return augment_patch_launch(a, (hipStream_t)stream);
}
extern "C" int ru_augment_patch(const float* image, const unsigned char* label, const float* mean, const float* inv_std, int C, int D, int H, int W,
                                const int* crop_lo, const int* patch, const double* scale, int flags, const float* gain, const float* bias,
                                float* data_out, float* target_out, ru_stream_t stream) {
    RU_REQUIRE(label, "ru_augment_patch: null argument");
    return augment_patch_impl(image, label, nullptr, mean, inv_std, C, D, H, W, crop_lo, patch, scale, flags, gain, bias, data_out, target_out, stream);
}
extern "C" int ru_augment_patch_soft(const float* image, const unsigned char* label, const float* soft, const float* mean, const float* inv_std, int C, int D, int H,
                                     int W, const int* crop_lo, const int* patch, const double* scale, int flags, const float* gain, const float* bias,
                                     float* data_out, float* target_out, ru_stream_t stream) {
    return augment_patch_impl(image, label, soft, mean, inv_std, C, D, H, W, crop_lo, patch, scale, flags, gain, bias, data_out, target_out, stream);
}
