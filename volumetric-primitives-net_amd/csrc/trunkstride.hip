// trunkstride.hip — the trunk's remaining convolutions (gfx950): square kernel R in {1, 3, 7}, any stride >= 1, any padding
// >= 0, dilation 1, groups 1, no bias, as an implicit GEMM on the f32-input MFMA, forward, data gradient and weight gradient
// (DESIGN.md 4.20).  The scheme is trunkconv.hip's, generalised.
//
// Replaces nn.Conv2d reached through the reference's vpnet_one_resnet.py:45-57 at the seven stride-2 sites of the ResNet-18
// trunk: the 7x7 stem, the three 3x3 layerN.0.conv1 and the three 1x1 layerN.0.downsample.0, forward and both gradients.
// NCHW contiguous, fp32 in, fp32 out.  OH = (H + 2 p - R) / st + 1 (floor), OW likewise.
//   * three products, ONE kernel template over (R, product).  GEMM view D[m][n] = sum_k A[m][k] B[k][n]:
//       forward          m = c_out, n = (b, oh, ow), k = (c_in, r, s):  A = w, B = x[b, c, oh st + r - p, ow st + s - p]
//       data gradient    m = c_in,  n = (b, ih, iw), k = (c_out, r, s): A = w read with the channel strides swapped,
//                        B = dy[b, co, (ih + p - r) / st, (iw + p - s) / st] where both quotients are exact and in range,
//                        else 0.0f (the masked form: every input pixel walks all R R taps; an input pixel that no output
//                        reads sums zeros alone and is written as 0)
//       weight gradient  m = c_out, n = (c_in, r, s), k = (b, oh, ow):  A = dy, B = x[b, c, oh st + r - p, ow st + s - p]
//     R is a template parameter, so k -> (c, r, s) is a division by a constant; stride and padding are arguments;
//   * the tile loop, the split of K over slices (over the generalised M, N, K), the merge of the partials and the one
//     summation order are vpn_conv_gemm.h's, shared with trunkconv.hip; the arguments, the taps, the data staging map and the
//     sizes are vpn_conv_stride.h's, shared with trunkfold.hip; this file holds the weight gradient's map and the table of
//     the products.  For R = 3, stride 1, padding 1 the k order is trunkconv.hip's: the results are bit-equal to
//     vpn_conv3x3_*;
//   * padding, stride gaps and the tails of all three GEMM dimensions are masked loads: an address is formed only for an
//     element that exists, everything else enters the product as 0.0f.
#include "vpn_conv_stride.h"

namespace vpn {

// weight gradient: k is the output pixel; both operands by (k fastest: 16 consecutive pixels of a channel)
template <int R>
struct CsWgradMap {
    static constexpr bool B_K_FASTEST = true;
    static constexpr unsigned RR = R * R;
    unsigned kk, am0, bn0;
    __device__ inline CsWgradMap(const CsArgs&, unsigned m0, unsigned n0, int tid) {
        kk = tid & 15; am0 = m0 + (tid >> 4); bn0 = n0 + (tid >> 4);
    }
    __device__ inline void load(const CsArgs& g, unsigned chunk, CgStage& st) const {
        const unsigned p = chunk * CG_K + kk;
        const bool pok = p < g.K;
        const unsigned b = pok ? p / g.PHW : 0, hw = pok ? p - b * g.PHW : 0;
        const int oh = hw / g.PW, ow = hw - oh * g.PW;
        const int h0 = oh * g.st - g.pad, w0 = ow * g.st - g.pad;
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (pok && m < g.M) ? g.a[((size_t)b * g.M + m) * g.PHW + hw] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned n = bn0 + 16 * j, c = n / RR, t = n - RR * c;
            const int r = t / R, s = t - R * r;
            st.b[j] = cs_tap_x(g, b, c, h0, w0, r, s, pok && n < g.N);
        }
    }
};

template <int R, int MODE> struct CsMapOf { typedef CsDataMap<R, MODE> type; };
template <int R> struct CsMapOf<R, CS_DW> { typedef CsWgradMap<R> type; };

// grid (tiles of N, tiles of M, S)
template <int R, int MODE>
__global__ __launch_bounds__(CG_BLOCK) void cs_gemm_kernel(CsArgs g) {
    cg_tile<typename CsMapOf<R, MODE>::type, MODE != CS_DW>(g);
}

// ---- the host side: one product (sizes and the GEMM view: vpn_conv_stride.h)
template <int R>
static void cs_launch(int product, const dim3& grid, hipStream_t st, const CsArgs& g) {
    if (product == VPN_CONV_FWD) VPN_LAUNCH_AS("cs_gemm_kernel<fwd>", (cs_gemm_kernel<R, CS_FWD>), grid, dim3(CG_BLOCK), 0, st, g);
    else if (product == VPN_CONV_DX) VPN_LAUNCH_AS("cs_gemm_kernel<dx>", (cs_gemm_kernel<R, CS_DX>), grid, dim3(CG_BLOCK), 0, st, g);
    else VPN_LAUNCH_AS("cs_gemm_kernel<dw>", (cs_gemm_kernel<R, CS_DW>), grid, dim3(CG_BLOCK), 0, st, g);
}

static int cs_run(int product, const CsDims& d, const CgPlan& p, const float* a, const float* b, float* out, void* ws, hipStream_t st) {
    const long long RR = (long long)d.R * d.R;
    CsArgs g;
    cg_fill(g, p, a, b, out, ws);
    g.CR = product == VPN_CONV_DX ? d.Cout : d.Cin;
    g.BH = product == VPN_CONV_DX ? d.OH : d.H; g.BW = product == VPN_CONV_DX ? d.OW : d.W;
    g.PW = product == VPN_CONV_DX ? d.W : d.OW; g.PHW = (product == VPN_CONV_DX ? d.H : d.OH) * g.PW;
    g.st = d.st; g.pad = d.pad;
    g.a_sm = product == VPN_CONV_FWD ? RR * d.Cin : RR; g.a_sk = product == VPN_CONV_FWD ? RR : RR * d.Cin;
    const dim3 grid(p.nt, p.mt, (unsigned)p.S);
    if (d.R == 1) cs_launch<1>(product, grid, st, g);
    else if (d.R == 3) cs_launch<3>(product, grid, st, g);
    else cs_launch<7>(product, grid, st, g);
    VPN_LAUNCH_CHECK();
    return cg_merge(p, ws, out, st);
}

}  // namespace vpn

using namespace vpn;

extern "C" int vpn_conv2d_splits(int B, int C_in, int C_out, int H, int W, int R, int stride, int pad, int product) {
    CsDims d;
    CgPlan p;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(product, d, &p);
    return rc ? rc : p.S;
}

extern "C" size_t vpn_conv2d_workspace(int B, int C_in, int C_out, int H, int W, int R, int stride, int pad, int products) {
    CsDims d;
    if (cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d) != 0) return 0;
    size_t need = 0;
    for (int product : {VPN_CONV_FWD, VPN_CONV_DX, VPN_CONV_DW}) {
        CgPlan p;
        if (!(products & product)) continue;
        if (cs_plan(product, d, &p) != 0) return 0;
        if (cg_ws_bytes(p) > need) need = cg_ws_bytes(p);
    }
    return need;
}

extern "C" int vpn_conv2d_fwd(const float* x, const float* w, float* y, int B, int C_in, int C_out, int H, int W, int R, int stride,
                              int pad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return VPN_E_BADARG;
    CsDims d;
    CgPlan p;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(VPN_CONV_FWD, d, &p);
    if (rc) return rc;
    if (cg_ws_bad(p, workspace, workspace_bytes)) return VPN_E_BADARG;
    return cs_run(VPN_CONV_FWD, d, p, w, x, y, workspace, (hipStream_t)stream);
}

extern "C" int vpn_conv2d_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int C_in, int C_out, int H,
                              int W, int R, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !w) return VPN_E_BADARG;
    CsDims d;
    CgPlan pd, pw;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(VPN_CONV_DX, d, &pd);
    if (!rc) rc = cs_plan(VPN_CONV_DW, d, &pw);
    if (rc) return rc;
    if ((dx && cg_ws_bad(pd, workspace, workspace_bytes)) || (dw && cg_ws_bad(pw, workspace, workspace_bytes)))
        return VPN_E_BADARG;
    // the two products use the workspace one after the other: launches of one stream run in order
    if (dx) { rc = cs_run(VPN_CONV_DX, d, pd, w, dy, dx, workspace, (hipStream_t)stream); if (rc) return rc; }
    if (dw) { rc = cs_run(VPN_CONV_DW, d, pw, dy, x, dw, workspace, (hipStream_t)stream); if (rc) return rc; }
    return 0;
}
