// conv3_pack_layout.hpp -- the ONE description of a packed split-bf16 3x3x3 weight: which fragment forms a pack buffer holds, where each starts, how many pack
// threads each takes and which of them a given pack request writes.  Everything that packs (conv3_sb.hip), sizes (conv3_sb_frag_bytes) or reads (conv3_sb_launch,
// conv3_wz_launch, sb2_cfg_m) a pack asks these functions; the per-form headers describe only what is INSIDE a form's units.
//
// A pack is a sequence of units of 64 lanes x 16 bytes.  The forms follow one another in the order of PackForm; a form the channel counts do not allow has no units,
// and the starts accumulate, so no form's place depends on another form being absent:
//   PF_DIRECT  three-product fragments of the direct kernels (sb_pack_one): every shape, per (16-cout group, 16-cin chunk) 14 K-steps x hi/lo
//   PF_HEAD    head form of the persistent kernel (sb_pack_head_one): at most 4 output and 16 input channels, 5 K-steps x hi/lo
//   PF_MX      fp16 + MX-fp8 form of the 16-channel level (mx_pack_one; activation OR gradient-operand variant, one of the two): 16 input channels, whole 16-cout groups
//   PF_WZ16    three-product Winograd-z form on 16x16x32 MFMAs (wz_pack_one; devtools builds only: the product library neither packs nor reserves it)
//   PF_WZ32    three-product Winograd-z form on 32x32x16 MFMAs (wz32_pack_one)      } >= 32 input channels in whole chunks,
//   PF_WZ32MX  fp16 + MX-fp8 Winograd-z form (wz32mx_pack_one)                      } whole 32-cout blocks
// Pack threads are numbered in the same order.  The direct range is always there (threads of a skipped direct form return at once); every other form takes threads
// only when it is requested -- but keeps its place in the buffer, whose bytes a skipped form leaves as they are.
#pragma once
#include <stddef.h>

namespace ru {

enum PackForm { PF_DIRECT = 0, PF_HEAD, PF_MX, PF_WZ16, PF_WZ32, PF_WZ32MX, PF_COUNT };
static inline const char* pack_form_name(int f) {
    static const char* const names[PF_COUNT + 2] = {"direct", "head", "mx", "wz16", "wz32", "wz32mx", "mx (gradient operand)", "4-channel"};
    return f >= 0 && f < PF_COUNT + 2 ? names[f] : "?";
}

// ---- a pack REQUEST (SbPackEntry::forms): which of the optional forms to write.  Frozen packs (inference, the op-level entries) must serve every later launch
// and ask for PACK_ALL; a training step repacks per forward and asks for what that forward's and its backward's launches read (sb_pack_forms).
constexpr int PACK_WZ16 = 1, PACK_WZ32 = 2, PACK_MX = 4, PACK_WZ32MX = 8;
constexpr int PACK_SKIP_DIRECT = 16;                    // the direct fragments are not written (no launch that reads this pack takes a direct kernel)
constexpr int PACK_MX_GRAD = 32;                        // the MX fragments in the gradient-operand variant, in the same place
constexpr int PACK_ALL = PACK_WZ16 | PACK_WZ32 | PACK_MX | PACK_WZ32MX;

// ---- what a pack HOLDS: bit f for every PackForm f written, PACK_HAS_MX_GRAD where the MX units are the gradient-operand variant (then without bit PF_MX), and
// PACK_HAS_SB4 for the separate buffer of the 4-channel kernel (conv3_sb4_pack_weights).  Travels with the pack pointer (Conv3Args::wforms, host only).
constexpr unsigned PACK_HAS_MX_GRAD = 1u << PF_COUNT, PACK_HAS_SB4 = 1u << (PF_COUNT + 1);

// ---- per-form geometry
constexpr int SB_KSTEPS = 14;                           // direct: ceil(27 taps / 2) K-steps
constexpr int SB_HEAD_KSTEPS = 5;
constexpr int MX_UNITS = 28;                            // per 16-cout group: 14 fp16 K-steps, 2 x 3 x 2 cross, 2 ninth chain
constexpr int WZ_KSTEPS = 5;
constexpr int WZ_UNITS = 4 * 2 * WZ_KSTEPS * 2;         // per (32-cout block, 16-cin chunk): [xi][group][K-step][hi/lo]
constexpr int WZ32_UNITS = 4 * 9 * 2;                   // [xi][tap dy*3+dx][hi/lo]
constexpr int WZ32MX_UNITS_XI = 9 + 5 * 2;              // per transformed plane: nine fp16 tap units, five cross units of two halves
constexpr int WZ32MX_UNITS = 4 * WZ32MX_UNITS_XI;
#ifdef RU_SB2_DBG
constexpr bool WZ16_FORM = true;
#else
constexpr bool WZ16_FORM = false;
#endif
__host__ __device__ constexpr bool sb_head_shape(int Cin_conv, int Cout_conv) { return Cout_conv <= 4 && Cin_conv <= 16; }
__host__ __device__ constexpr bool mx_channels_ok(int Cin_conv, int Cout_conv) { return Cin_conv == 16 && Cout_conv % 16 == 0; }
// channel counts for which the transformed fragments exist beside the direct ones (whether a SHAPE takes the kernel: conv3_wz_shape_ok)
__host__ __device__ constexpr bool wz_channels_ok(int Cin_conv, int Cout_conv) { return Cin_conv >= 32 && Cin_conv % 16 == 0 && Cout_conv % 32 == 0; }

// units and pack threads of ONE block of a form (a pack thread writes one lane of 1, 2 or 4 units), and the request bit that asks for it (0: always packed)
struct PackFormRule { int units, threads, request; };
__host__ __device__ constexpr PackFormRule pack_form_rule(int f) {
    return f == PF_DIRECT ? PackFormRule{SB_KSTEPS * 2, SB_KSTEPS * 64, 0}
         : f == PF_HEAD   ? PackFormRule{SB_HEAD_KSTEPS * 2, SB_HEAD_KSTEPS * 64, 0}
         : f == PF_MX     ? PackFormRule{MX_UNITS, MX_UNITS * 64, PACK_MX}
         : f == PF_WZ16   ? PackFormRule{WZ_UNITS, WZ_UNITS / 2 * 64, PACK_WZ16}
         : f == PF_WZ32   ? PackFormRule{WZ32_UNITS, WZ32_UNITS / 2 * 64, PACK_WZ32}
                          : PackFormRule{WZ32MX_UNITS, WZ32MX_UNITS_XI * 64, PACK_WZ32MX};
}
// blocks of form f in the pack of a (cin_conv -> cout_conv) weight; 0: the channel counts have no such form
__host__ __device__ constexpr int pack_form_blocks(int f, int cin_conv, int cout_conv) {
    const int nchunk = (cin_conv + 15) / 16, ncog = (cout_conv + 15) / 16;
    return f == PF_DIRECT ? ncog * nchunk
         : f == PF_HEAD   ? (sb_head_shape(cin_conv, cout_conv) ? 1 : 0)
         : f == PF_MX     ? (mx_channels_ok(cin_conv, cout_conv) ? ncog : 0)
         : f == PF_WZ16 && !WZ16_FORM ? 0
                          : (wz_channels_ok(cin_conv, cout_conv) ? (cout_conv / 32) * nchunk : 0);
}

constexpr size_t PACK_UNIT_BYTES = 64 * 16;
struct PackLayout {
    size_t start[PF_COUNT];                             // in units
    int units[PF_COUNT];                                // 0: absent
    size_t total;                                       // in units
};
__host__ __device__ inline PackLayout pack_layout(int cin_conv, int cout_conv) {
    PackLayout L{};
    for (int f = 0; f < PF_COUNT; ++f) {
        L.start[f] = L.total;
        L.units[f] = pack_form_blocks(f, cin_conv, cout_conv) * pack_form_rule(f).units;
        L.total += (size_t)L.units[f];
    }
    return L;
}
// pack thread range [begin, begin + count) of every form under the request `forms`
struct PackThreads { int begin[PF_COUNT], count[PF_COUNT], total; };
__host__ __device__ inline PackThreads pack_threads(int cin_conv, int cout_conv, int forms) {
    PackThreads T{};
    for (int f = 0; f < PF_COUNT; ++f) {
        const PackFormRule r = pack_form_rule(f);
        T.begin[f] = T.total;
        T.count[f] = (r.request == 0 || (forms & r.request)) ? pack_form_blocks(f, cin_conv, cout_conv) * r.threads : 0;
        T.total += T.count[f];
    }
    return T;
}
// the forms-present word of a pack written under the request `forms`
static inline unsigned pack_forms_present(int cin_conv, int cout_conv, int forms) {
    const PackThreads T = pack_threads(cin_conv, cout_conv, forms);
    unsigned has = 0;
    for (int f = 0; f < PF_COUNT; ++f)
        if (T.count[f] > 0) has |= 1u << f;
    if (forms & PACK_SKIP_DIRECT) has &= ~(1u << PF_DIRECT);
    if ((has >> PF_MX & 1u) && (forms & PACK_MX_GRAD)) has = (has & ~(1u << PF_MX)) | PACK_HAS_MX_GRAD;
    return has;
}
// start of form f inside the pack at `wfrag`
template <class T>
static inline T* pack_form_ptr(T* wfrag, int cin_conv, int cout_conv, PackForm f) {
    return reinterpret_cast<T*>((size_t)wfrag + pack_layout(cin_conv, cout_conv).start[f] * PACK_UNIT_BYTES);
}

}  // namespace ru
