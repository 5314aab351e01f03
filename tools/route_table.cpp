// route_table.cpp -- the kernel choice of the 3x3x3 split-bf16 family as a table: for every setting of the kernel-choice switches (csrc/switches.hpp) and a grid
// of argument sets, the route (conv3_sb_route), the partial count that follows from it (conv3_sb_route_nblk), the plan predicates and the fragment forms a
// training forward / backward packs.  Host only: no GPU call (without a device sb_ncu() answers 256 compute units, the MI355X's count).  A change that is meant
// to leave the routing alone is checked by building this against the library before and after it and comparing the two outputs byte for byte.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 tools/route_table.cpp -o route_table -Lbrats2019_amd/lib -lresunet_hip -Wl,-rpath,$PWD/brats2019_amd/lib
//   ./route_table > table.txt          (about 130 MB; the last line is an FNV-1a hash of everything above it)
#include "../brats2019_amd/csrc/ru_common.h"

#include <stdlib.h>
#include <string>

using namespace ru;

static unsigned long long g_hash = 1469598103934665603ull;
static void emit(const std::string& line) {
    for (unsigned char c : line) { g_hash ^= c; g_hash *= 1099511628211ull; }
    fputs(line.c_str(), stdout);
}
static void env(const char* name, const char* value) { if (value) setenv(name, value, 1); else unsetenv(name); }

int main() {
    static float some;                                    // the route tests pointers for null only
    const char* wz_v[] = {nullptr, "0"};
    const char* mx_v[] = {nullptr, "0", "1"};
    const int Ns[] = {1, 2, 4};
    const int ch[][2] = {{4, 16}, {16, 16}, {32, 32}, {64, 64}, {128, 128}, {16, 3}, {3, 16}, {32, 16}};
    const int shp[][3] = {{8, 8, 8}, {16, 16, 16}, {32, 32, 32}, {64, 64, 64}, {128, 128, 128}, {5, 6, 8}};
    char buf[256];
    for (const char* wz : wz_v) for (const char* mx : mx_v) for (const char* mxg : wz_v) for (const char* hf : wz_v) for (const char* hr : wz_v) {
        env("RU_WZ", wz); env("RU_MX", mx); env("RU_MXG", mxg); env("RU_HEAD_FORM", hf); env("RU_HEAD_RES", hr);
        const Switches sw = switches_from_env();
        snprintf(buf, sizeof(buf), "== RU_WZ=%s RU_MX=%s RU_MXG=%s RU_HEAD_FORM=%s RU_HEAD_RES=%s\n", wz ? wz : "-", mx ? mx : "-", mxg ? mxg : "-", hf ? hf : "-", hr ? hr : "-");
        emit(buf);
        for (int N : Ns) for (const auto& c : ch) for (const auto& d : shp) {
            const int Cin = c[0], Cout = c[1], D = d[0], H = d[1], W = d[2];
            // the plan: what the engine asks before it builds its arguments, and what a training step packs of this weight at this shape
            Conv3Args fwd{};                              // the forward launch of the engine's voxel-major flow that reads the weight (engine.hip, conv3_gn_args)
            fwd.mode = RU_PREC_BF16X3; fwd.N = N; fwd.Cin = Cin; fwd.Cout = Cout; fwd.D = D; fwd.H = H; fwd.W = W; fwd.in_c16 = 1; fwd.out_c16 = 1; fwd.products = 2;
            const bool skip_direct = conv3_route_skips_direct(conv3_sb_route(fwd, sw));
            // forward weight without / with the engine's PACK_SKIP_DIRECT, data-gradient weight
            const int forms[3] = {sb_pack_forms(sw, 0), sb_pack_forms(sw, 0) | (skip_direct ? PACK_SKIP_DIRECT : 0), sb_pack_forms(sw, 1)};
            snprintf(buf, sizeof(buf), "N=%d %d->%d %dx%dx%d plan: head_res=%d mxg=%d skip_direct=%d forms=%d/%d/%d\n", N, Cin, Cout, D, H, W,
                     (int)conv3_sb_head_takes_residual(sw, N, Cin, Cout, D, H, W), (int)conv3_mxg_usable(sw, N, Cin, Cout, D, H, W),
                     (int)skip_direct, forms[0], forms[1], forms[2]);
            emit(buf);
            // layouts: bit 0 voxel-major input, bit 1 voxel-major output; the 4-channel copy exists for NCDHW inputs of <= 4 channels, the split / gradient-operand
            // forms for voxel-major inputs
            for (int lay = 0; lay < 4; ++lay) for (int inform = 0; inform < 3; ++inform) for (int products = 0; products < 3; ++products) {
                const bool in16 = lay & 1;
                if (inform && !in16 && !(inform == 1 && Cin <= 4)) continue;
                Conv3Args a{};
                a.mode = RU_PREC_BF16X3; a.N = N; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W;
                a.in_c16 = in16; a.out_c16 = (lay >> 1) & 1; a.products = products;
                if (in16) { a.in_s16 = inform >= 1; a.in_g16 = inform == 2; } else a.in_c4 = inform == 1;
                std::string line;
                snprintf(buf, sizeof(buf), " in16=%d out16=%d c4=%d s16=%d g16=%d products=%d:", a.in_c16, a.out_c16, a.in_c4, a.in_s16, a.in_g16, products);
                line = buf;
                for (int f = 0; f < 64; ++f) {            // bit 0 add, 1 bst_y, 2 bias, 3 sigmoid, 4 in_res, 5 stat_partials
                    a.add = (f & 1) ? &some : nullptr; a.bst_y = (f & 2) ? &some : nullptr; a.bst_k = a.bst_y; a.bias = (f & 4) ? &some : nullptr;
                    a.sigmoid = (f >> 3) & 1; a.in_res = (f & 16) ? &some : nullptr; a.stat_partials = (f & 32) ? &some : nullptr;
                    const int r = conv3_sb_route(a, sw);
                    snprintf(buf, sizeof(buf), " %x/%d", r, conv3_sb_route_nblk(r, N, Cout, D, H, W));
                    line += buf;
                }
                emit(line + "\n");
            }
        }
    }
    printf("fnv1a %016llx\n", g_hash);
    return 0;
}
