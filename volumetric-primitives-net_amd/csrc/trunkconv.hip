// trunkconv.hip — the trunk's 3x3 convolutions (gfx950): kernel 3x3, stride 1, padding 1, dilation 1, groups 1, no bias, as
// an implicit GEMM on the f32-input MFMA, forward, data gradient and weight gradient.
//
// Replaces nn.Conv2d inside torchvision's BasicBlock, reached through the reference's vpnet_one_resnet.py:45-57: 13 of the
// 20 convolutions of the ResNet-18 trunk, forward and both gradients.  NCHW contiguous, fp32 in, fp32 out.
//   * three products, ONE kernel template.  GEMM view D[m][n] = sum_k A[m][k] B[k][n]:
//       forward          m = c_out, n = (b, h, w), k = (c_in, r, s):  A = w, B = x shifted by (r - 1, s - 1)
//       data gradient    m = c_in,  n = (b, h, w), k = (c_out, r, s): A = w read with the channel strides swapped, B = dy
//                        shifted by (1 - r, 1 - s): the same code, other strides and a sign; no transposed copy of w
//       weight gradient  m = c_out, n = (c_in, r, s), k = (b, h, w):  A = dy, B = x shifted by (r - 1, s - 1)
//   * the tile loop, the split of K over slices, the merge of the partials and the one summation order are
//     vpn_conv_gemm.h's, shared with trunkstride.hip; this file holds the two staging maps and the table of the products;
//   * padding, and the tails of all three GEMM dimensions, are masked loads: an address is formed only for an element that
//     exists, everything else enters the product as 0.0f;
//   * the operand loads are element loads, consecutive lanes on consecutive addresses (the shifted taps of a row start at
//     w - 1, w, w + 1: never all 16-byte aligned).
#include "vpn_conv_gemm.h"
#include <type_traits>

namespace vpn {

enum { CV_DATA = 0, CV_WGRAD = 1 };

struct CvArgs {
    const float* a;            // CV_DATA: the weights [C_out, C_in, 3, 3]; CV_WGRAD: dy [B, M, H, W]
    const float* b;            // CV_DATA: x (forward) or dy (data gradient) [B, CR, H, W]; CV_WGRAD: x [B, CR, H, W]
    float* out;                // the result, or the workspace [S][total] when S > 1
    unsigned M, N, K;          // the GEMM's sizes
    int CR;                    // channels of `b`: CV_DATA K = 9 CR, CV_WGRAD N = 9 CR
    int H, W, PHW;             // the image; PHW = H W
    long long a_sm, a_sk;      // CV_DATA: strides of w for the m channel and the reduction channel
    int flip;                  // CV_DATA: 1 mirrors the taps (data gradient)
    int chunks, S;             // chunks of CG_K in K; slices
    long long total;           // elements of the result: the pitch of a partial in the workspace
};

// (r - 1, s - 1) of tap rs, mirrored for the data gradient
__device__ inline void cv_tap(int rs, int flip, int& dh, int& dw) {
    const int r = rs / 3, s = rs - 3 * r;
    dh = flip ? 1 - r : r - 1;
    dw = flip ? 1 - s : s - 1;
}

// the image element (b, c, h + dh, w + dw) of a [B, C, H, W] tensor, 0 outside the image: no address is formed there
__device__ inline float cv_pixel(const float* t, const CvArgs& g, unsigned b, unsigned c, int h, int w, int dh, int dw, bool ok) {
    const int ih = h + dh, iw = w + dw;
    if (!ok || ih < 0 || ih >= g.H || iw < 0 || iw >= g.W) return 0.0f;
    return t[(((size_t)b * g.CR + c) * g.H + ih) * g.W + iw];
}

// CV_DATA: A by (k fastest: 16 consecutive weights of a row forward), B by (pixel fastest: 64 consecutive pixels of a tap)
struct CvDataMap {
    static constexpr bool B_K_FASTEST = false;
    unsigned ak, am0, bn, bk0, nb; int nh, nw; bool nok;
    __device__ inline CvDataMap(const CvArgs& g, unsigned m0, unsigned n0, int tid) {
        ak = tid & 15; am0 = m0 + (tid >> 4);
        bn = n0 + (tid & 63); bk0 = tid >> 6;
        nok = bn < g.N;
        nb = nok ? bn / g.PHW : 0;
        const unsigned hw = nok ? bn - nb * g.PHW : 0;
        nh = hw / g.W; nw = hw - nh * g.W;
    }
    __device__ inline void load(const CvArgs& g, unsigned chunk, CgStage& st) const {
        const unsigned k = chunk * CG_K + ak, kc = k / 9, rs = k - 9 * kc;
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (k < g.K && m < g.M) ? g.a[(size_t)m * g.a_sm + (size_t)kc * g.a_sk + rs] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned kb = chunk * CG_K + bk0 + 4 * j, c = kb / 9;
            int dh, dw;
            cv_tap(kb - 9 * c, g.flip, dh, dw);
            st.b[j] = cv_pixel(g.b, g, nb, c, nh, nw, dh, dw, nok && kb < g.K);
        }
    }
};

// CV_WGRAD: k is the pixel; both operands by (k fastest: 16 consecutive pixels of a channel)
struct CvWgradMap {
    static constexpr bool B_K_FASTEST = true;
    unsigned kk, am0, bn0;
    __device__ inline CvWgradMap(const CvArgs&, unsigned m0, unsigned n0, int tid) {
        kk = tid & 15; am0 = m0 + (tid >> 4); bn0 = n0 + (tid >> 4);
    }
    __device__ inline void load(const CvArgs& g, unsigned chunk, CgStage& st) const {
        const unsigned p = chunk * CG_K + kk;
        const bool pok = p < g.K;
        const unsigned b = pok ? p / g.PHW : 0, hw = pok ? p - b * g.PHW : 0;
        const int h = hw / g.W, w = hw - h * g.W;
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (pok && m < g.M) ? g.a[((size_t)b * g.M + m) * g.PHW + hw] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned n = bn0 + 16 * j, c = n / 9;
            int dh, dw;
            cv_tap(n - 9 * c, 0, dh, dw);
            st.b[j] = cv_pixel(g.b, g, b, c, h, w, dh, dw, pok && n < g.N);
        }
    }
};

// grid (tiles of N, tiles of M, S)
template <int MODE>
__global__ __launch_bounds__(CG_BLOCK) void cv_gemm_kernel(CvArgs g) {
    cg_tile<typename std::conditional<MODE == CV_DATA, CvDataMap, CvWgradMap>::type, MODE == CV_DATA>(g);
}

// ---- the host side: sizes and the GEMM view of one product
static int cv_plan(int product, int B, int Cin, int Cout, int H, int W, CgPlan* p) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    const long long HW = (long long)H * W, lim = 2147483647LL;
    if (HW > lim || HW * B > lim || HW * B * Cin > lim || HW * B * Cout > lim || 9LL * Cin * Cout > lim) return VPN_E_TOOBIG;
    const unsigned P = (unsigned)B * H * W;
    if (product == VPN_CONV_FWD) return cg_plan(Cout, P, 9u * Cin, (long long)P * Cout, p);
    if (product == VPN_CONV_DX) return cg_plan(Cin, P, 9u * Cout, (long long)P * Cin, p);
    if (product == VPN_CONV_DW) return cg_plan(Cout, 9u * Cin, P, 9LL * Cin * Cout, p);
    return VPN_E_BADARG;
}

static int cv_run(int product, const CgPlan& p, const float* a, const float* b, float* out, int Cin, int Cout, int H, int W, void* ws,
                  hipStream_t st) {
    CvArgs g;
    cg_fill(g, p, a, b, out, ws);
    g.CR = product == VPN_CONV_DX ? Cout : Cin; g.H = H; g.W = W; g.PHW = H * W;
    g.a_sm = product == VPN_CONV_FWD ? 9LL * Cin : 9; g.a_sk = product == VPN_CONV_FWD ? 9 : 9LL * Cin;
    g.flip = product == VPN_CONV_DX;
    const dim3 grid(p.nt, p.mt, (unsigned)p.S);
    if (product == VPN_CONV_DW) VPN_LAUNCH_AS("cv_gemm_kernel<wgrad>", (cv_gemm_kernel<CV_WGRAD>), grid, dim3(CG_BLOCK), 0, st, g);
    else VPN_LAUNCH_AS("cv_gemm_kernel<data>", (cv_gemm_kernel<CV_DATA>), grid, dim3(CG_BLOCK), 0, st, g);
    VPN_LAUNCH_CHECK();
    return cg_merge(p, ws, out, st);
}

}  // namespace vpn

using namespace vpn;

extern "C" int vpn_conv3x3_splits(int B, int C_in, int C_out, int H, int W, int product) {
    CgPlan p;
    const int rc = cv_plan(product, B, C_in, C_out, H, W, &p);
    return rc ? rc : p.S;
}

extern "C" size_t vpn_conv3x3_workspace(int B, int C_in, int C_out, int H, int W, int products) {
    size_t need = 0;
    for (int product : {VPN_CONV_FWD, VPN_CONV_DX, VPN_CONV_DW}) {
        CgPlan p;
        if (!(products & product)) continue;
        if (cv_plan(product, B, C_in, C_out, H, W, &p) != 0) return 0;
        if (cg_ws_bytes(p) > need) need = cg_ws_bytes(p);
    }
    return need;
}

extern "C" int vpn_conv3x3_fwd(const float* x, const float* w, float* y, int B, int C_in, int C_out, int H, int W, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return VPN_E_BADARG;
    CgPlan p;
    const int rc = cv_plan(VPN_CONV_FWD, B, C_in, C_out, H, W, &p);
    if (rc) return rc;
    if (cg_ws_bad(p, workspace, workspace_bytes)) return VPN_E_BADARG;
    return cv_run(VPN_CONV_FWD, p, w, x, y, C_in, C_out, H, W, workspace, (hipStream_t)stream);
}

extern "C" int vpn_conv3x3_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int C_in, int C_out, int H,
                               int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !w) return VPN_E_BADARG;
    CgPlan pd, pw;
    int rc = cv_plan(VPN_CONV_DX, B, C_in, C_out, H, W, &pd);
    if (!rc) rc = cv_plan(VPN_CONV_DW, B, C_in, C_out, H, W, &pw);
    if (rc) return rc;
    if ((dx && cg_ws_bad(pd, workspace, workspace_bytes)) || (dw && cg_ws_bad(pw, workspace, workspace_bytes)))
        return VPN_E_BADARG;
    // the two products use the workspace one after the other: launches of one stream run in order
    if (dx) { rc = cv_run(VPN_CONV_DX, pd, w, dy, dx, C_in, C_out, H, W, workspace, (hipStream_t)stream); if (rc) return rc; }
    if (dw) { rc = cv_run(VPN_CONV_DW, pw, dy, x, dw, C_in, C_out, H, W, workspace, (hipStream_t)stream); if (rc) return rc; }
    return 0;
}
