// vpn_head_rule.h — the per-field rule of restrict_range + restrict_volumes (modules/network/vpnet_one_resnet.py:67-85 of
// the reference), shared by head.hip (vpn_head_pack_*) and fcstack.hip (the vp_pack epilogue of vpn_fc_stack_*): one
// definition, so the two kernels cannot drift apart.
#pragma once
#include "vpn_common.h"

namespace vpn {

__device__ inline float sigmoidf(float x) {                     // overflow-free on both sides
    const float e = __expf(-fabsf(x));
    const float s = 1.0f / (1.0f + e);
    return x >= 0.0f ? s : e * s;
}

struct HeadRule { int is_sigmoid; float cmin, cmax, r0, r1, r2; };

// field f of a packed row (0..2 volumes, 3..6 rotates, 7..9 translates): raw head output x -> value y, dy = dy/dx
__device__ inline void head_field(const HeadRule& h, int f, float x, float& y, float& dy) {
    if (h.is_sigmoid) {
        if (f < 7) { const float s = sigmoidf(x); y = f < 3 ? s + 0.1f : s; dy = s * (1.0f - s); }     // :70-71
        else { y = tanhf(x); dy = 1.0f - y * y; }                                                        // :72
    } else {
        const float lo = f < 3 ? h.cmin + 1e-8f : -1.0f, hi = f < 3 ? h.cmax : 1.0f;                      // :74-76
        y = fminf(fmaxf(x, lo), hi);
        dy = (x >= lo && x <= hi) ? 1.0f : 0.0f;                 // torch.clamp passes the gradient on the closed interval
    }
    if (f < 3) { const float r = f == 0 ? h.r0 : (f == 1 ? h.r1 : h.r2); y = y / r; dy = dy / r; }        // :81-84
}

}  // namespace vpn
