// switches.hpp -- every environment variable the library reads, and the one value the kernel choice of the 3x3x3 family depends on.
//
// The environment is the source (bench.py, the A/B scripts of tools/ and the tests set it); engine.hip holds the only reads of it.  A public entry that can
// reach a 3x3x3 launch, pack or plan takes ONE Switches value on entry (switches_from_env) and hands it down: routes, pack forms, partial counts and the
// backward's pack check are pure functions of their arguments and that value.  A switch is OFF when its variable starts with the character named below.
//
// | variable            | default | read                    | selects                                                                                         |
// |---------------------|---------|-------------------------|-------------------------------------------------------------------------------------------------|
// | RU_WZ               | on      | per public call         | 0: every 3x3x3 convolution stays on the direct kernels (default: the voxel-major forward ones   |
// |                     |         |                         | of 32.. channels whose shape fills the chip take the Winograd-z kernels) -> Switches::wz        |
// | RU_WZ32             | on      | per public call,        | 0: the Winograd-z launches take the 16x16x32 matrix form (conv3_wz_kernel) instead of           |
// |                     |         | devtools builds only    | conv3_wz32_kernel; the product library has no such form and ignores it -> Switches::wz32        |
// | RU_MX               | on      | per public call         | 0: forward convolutions keep three bf16 products (Switches::mx and mx_wz off);                  |
// |                     |         |                         | 1: the fp16 + MX-fp8 scheme at the 16-channel level only, conv3_mx_kernel (mx_wz off);          |
// |                     |         |                         | default: also its Winograd-z form at 32.. channels, conv3_wz32mx_kernel                         |
// | RU_MXG              | on      | per public call         | 0: the 16-channel data-gradient convolutions keep three bf16 products over the split form       |
// |                     |         |                         | (default: conv3_mx_kernel<GRAD> on the gradient-operand form) -> Switches::mxg                  |
// | RU_HEAD_FORM        | on      | per public call         | 0: the <= 4-output-channel convolutions stay on the 16-column kernel -> Switches::head_form     |
// | RU_HEAD_RES         | on      | per public call         | 0: the last block's residual pass runs by itself (default: the head conv's staging forms it,    |
// |                     |         |                         | Conv3Args::in_res; bit-identical) -> Switches::head_res                                         |
// | RU_F32C             | on      | once per process        | 0: the exact-f32 inference forward keeps the NCDHW flow                                         |
// | RU_TRACE            | off     | once per process        | 1: every launch of the executor is named on stderr and followed by a stream synchronisation     |
// | RU_SB1_NO22         | off     | once per process        | 1: sb_choose never picks the half-size (2,2,16) tile of the one-stage kernel (tools)            |
// | RU_C1_SCATTER_COB   | 0       | once per process        | 1 / 2 / 4: output channel blocks per workgroup of the scattering 1x1 convolution (tools)        |
// | RU_C1_PAIR          | on      | once per process        | 0: the scattering 1x1 convolution keeps its plain epilogue (bit-identical)                      |
// | RU_SIDE_STREAM      | on      | once per ru_unet_create | 0: clears RU_FUSE_SIDE_STREAM in the handle's fusion mask                                       |
// | RU_FUSION_OFF       | 0       | once per ru_unet_create | a mask of RU_FUSE_* bits to clear                                                               |
// | RU_FUSION_ON        | 0       | once per ru_unet_create | a mask of RU_FUSE_* bits to set (the opt-in ones)                                               |
#pragma once

namespace ru {

struct Switches {
    bool wz = true, wz32 = true, mx = true, mx_wz = true, mxg = true, head_form = true, head_res = true;
    // the fields that select which fragment forms a training step packs (the head switches select none: a head shape always packs its SB_HEAD_KSTEPS fragments)
    int pack_bits() const { return (wz ? 1 : 0) | (wz32 ? 2 : 0) | (mx ? 4 : 0) | (mx_wz ? 8 : 0) | (mxg ? 16 : 0); }
    bool operator==(const Switches& o) const { return pack_bits() == o.pack_bits() && head_form == o.head_form && head_res == o.head_res; }
};
Switches switches_from_env();

bool env_trace();
bool env_f32c_off();
bool env_sb1_no22();
int env_c1_scatter_cob();
bool env_c1_pair_off();
unsigned env_fusion(unsigned fusion);       // the fusion mask of a new handle after RU_SIDE_STREAM / RU_FUSION_OFF / RU_FUSION_ON

}  // namespace ru
