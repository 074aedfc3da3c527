// trunkfold.hip — the trunk's convolutions for eval-mode inference (gfx950): y = act(conv(x, w) + bias[c_out] + residual), a
// batch norm folded into the weights and a per-channel bias, the residual add and the ReLU in the convolution's epilogue.
// Forward only.
//
// Replaces nn.Conv2d + nn.BatchNorm2d (eval) + add + ReLU reached through the reference's vpnet_one_resnet.py:45-57: all 20
// convolution sites of the ResNet-18 trunk when nothing is trained (train_gcn.py:100-125, test.py, test_gcn.py).  NCHW
// contiguous, fp32 in, fp32 out.  Square kernel R in {1, 3, 7}, any stride >= 1, any padding >= 0.
//   * the product is trunkstride.hip's forward: the same GEMM view (m = c_out, n = (b, oh, ow), k = (c_in, r, s)), the same
//     staging map CsDataMap<R, CS_FWD> with its masked loads (vpn_conv_stride.h), the tile loop, plan, split rule and k order
//     of vpn_conv_gemm.h.  With no bias, no residual and no ReLU the result is vpn_conv2d_fwd's bit for bit;
//   * unsplit (S = 1): the epilogue runs at cg_tile's store, per accumulator register, the channel being the row m:
//     v = acc + bias[m]; v += residual[idx]; v = v < 0 ? 0 : v (a NaN stays a NaN).  One launch;
//   * split (S > 1): the GEMM writes raw partials to the workspace, cf_merge_kernel adds them in the order 0 .. S - 1 and
//     applies the same three steps in the same order; the channel of element u is (u / PHW) % M.  16-byte accesses when the
//     element count is a multiple of 4 and y and the residual are 16-byte aligned (a float4 may hold two channels: each of
//     its elements finds its own), element accesses otherwise.  Two launches;
//   * bias, residual and relu are runtime arguments, a null pointer means absent: one GEMM kernel per R, the merge by 4 and
//     by 1.  No atomics, no grid barrier, nothing allocated, no host synchronisation: bit-equal from run to run, capturable.
#include "vpn_conv_stride.h"

namespace vpn {

struct CfArgs : CsArgs {
    const float* bias;         // [M] or null
    const float* res;          // the result's shape or null
    int relu;
};

// bias, residual, ReLU of one element of channel m, in that order
__device__ __forceinline__ float cf_finish(float v, const float* bias, const float* res, int relu, unsigned m, size_t idx) {
    if (bias) v += bias[m];
    if (res) v += res[idx];
    if (relu) v = v < 0.0f ? 0.0f : v;
    return v;
}

// cg_tile's store: a slice of a split product leaves its partial raw, the merge finishes it
struct CfStore {
    __device__ static __forceinline__ void store(const CfArgs& g, float* out, size_t idx, unsigned m, float v) {
        out[idx] = g.S > 1 ? v : cf_finish(v, g.bias, g.res, g.relu, m, idx);
    }
};

// grid (tiles of N, tiles of M, S)
template <int R>
__global__ __launch_bounds__(CG_BLOCK) void cf_gemm_kernel(CfArgs g) {
    cg_tile<CsDataMap<R, CS_FWD>, true, CfStore>(g);
}

struct CfTail { const float* bias; unsigned M, PHW; int relu; };

// r += bias of its channel: element e of the result is of channel (e / PHW) % M; a float4 may hold two channels
__device__ inline float cf_bias_of(const CfTail& t, unsigned e) { return t.bias[e / t.PHW % t.M]; }
__device__ inline void cf_bias(float& r, long long u, const CfTail& t) { r += cf_bias_of(t, (unsigned)u); }
__device__ inline void cf_bias(float4& r, long long u, const CfTail& t) {
    const unsigned e = 4u * (unsigned)u;
    r.x += cf_bias_of(t, e); r.y += cf_bias_of(t, e + 1); r.z += cf_bias_of(t, e + 2); r.w += cf_bias_of(t, e + 3);
}

__device__ inline void cf_relu(float& r) { r = r < 0.0f ? 0.0f : r; }
__device__ inline void cf_relu(float4& r) { cf_relu(r.x); cf_relu(r.y); cf_relu(r.z); cf_relu(r.w); }

// out[u] = act(ws[0][u] + ws[1][u] + ... + ws[S - 1][u] + bias + res[u]), the partials in that order, then the epilogue's
// three steps in theirs, for `units` elements of T (float, or float4 for 16-byte accesses); `pitch`: the elements of T in a
// partial
template <class T>
__global__ __launch_bounds__(CG_BLOCK) void cf_merge_kernel(const T* ws, const T* res, T* out, long long units, long long pitch, int S,
                                                            CfTail t) {
    const long long u = (long long)blockIdx.x * CG_BLOCK + threadIdx.x;
    if (u >= units) return;
    T r = ws[u];
    for (int s = 1; s < S; ++s) cg_add(r, ws[(size_t)s * pitch + u]);
    if (t.bias) cf_bias(r, u, t);
    if (res) cg_add(r, res[u]);
    if (t.relu) cf_relu(r);
    out[u] = r;
}

static int cf_run(const CsDims& d, const CgPlan& p, const float* x, const float* w, const float* bias, const float* res, float* y,
                  int relu, void* ws, hipStream_t st) {
    const long long RR = (long long)d.R * d.R;
    CfArgs g;
    cg_fill(g, p, w, x, y, ws);
    g.CR = d.Cin; g.BH = d.H; g.BW = d.W; g.PW = d.OW; g.PHW = d.OH * d.OW;
    g.st = d.st; g.pad = d.pad;
    g.a_sm = RR * d.Cin; g.a_sk = RR;
    g.bias = bias; g.res = res; g.relu = relu;
    const dim3 grid(p.nt, p.mt, (unsigned)p.S);
    if (d.R == 1) VPN_LAUNCH_AS("cf_gemm_kernel", (cf_gemm_kernel<1>), grid, dim3(CG_BLOCK), 0, st, g);
    else if (d.R == 3) VPN_LAUNCH_AS("cf_gemm_kernel", (cf_gemm_kernel<3>), grid, dim3(CG_BLOCK), 0, st, g);
    else VPN_LAUNCH_AS("cf_gemm_kernel", (cf_gemm_kernel<7>), grid, dim3(CG_BLOCK), 0, st, g);
    VPN_LAUNCH_CHECK();
    if (p.S == 1) return 0;
    // the workspace is 16-byte aligned (checked)
    const bool vec = p.total % 4 == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)res & 15) == 0;
    const long long units = vec ? p.total / 4 : p.total;
    const dim3 mg((unsigned)((units + CG_BLOCK - 1) / CG_BLOCK));
    const CfTail t = {bias, p.M, (unsigned)g.PHW, relu};
    if (vec) VPN_LAUNCH_AS("cf_merge_kernel", (cf_merge_kernel<float4>), mg, dim3(CG_BLOCK), 0, st, (const float4*)ws, (const float4*)res, (float4*)y, units, units, p.S, t);
    else VPN_LAUNCH_AS("cf_merge_kernel", (cf_merge_kernel<float>), mg, dim3(CG_BLOCK), 0, st, (const float*)ws, res, y, units, units, p.S, t);
    VPN_LAUNCH_CHECK();
    return 0;
}

}  // namespace vpn

using namespace vpn;

extern "C" int vpn_conv2d_bias_act_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int C_in,
                                       int C_out, int H, int W, int R, int stride, int pad, int relu, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return VPN_E_BADARG;
    if (relu != 0 && relu != 1) return VPN_E_BADARG;
    CsDims d;
    CgPlan p;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(VPN_CONV_FWD, d, &p);
    if (rc) return rc;
    if (cg_ws_bad(p, workspace, workspace_bytes)) return VPN_E_BADARG;
    return cf_run(d, p, x, w, bias, residual, y, relu, workspace, (hipStream_t)stream);
}
