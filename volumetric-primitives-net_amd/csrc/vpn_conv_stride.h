// vpn_conv_stride.h — what csrc/trunkstride.hip and csrc/trunkfold.hip share of the general convolution (square kernel R in
// {1, 3, 7}, any stride >= 1, any padding >= 0): the kernel arguments, the masked taps, the staging map of
// the forward and the data gradient, and the host side's sizes and GEMM view.  The tile loop, the plan and the split rule are
// vpn_conv_gemm.h's.
#pragma once
#include "vpn_conv_gemm.h"

namespace vpn {

enum { CS_FWD = 0, CS_DX = 1, CS_DW = 2 };

struct CsArgs {
    const float* a;            // forward, data gradient: the weights [C_out, C_in, R, R]; weight gradient: dy [B, M, OH, OW]
    const float* b;            // forward, weight gradient: x [B, CR, BH, BW]; data gradient: dy [B, CR, BH, BW]
    float* out;                // the result, or the workspace [S][total] when S > 1
    unsigned M, N, K;          // the GEMM's sizes
    int CR;                    // channels of `b`
    int BH, BW;                // image of `b`: H x W of x, or OH x OW of dy for the data gradient
    int PW, PHW;               // width and size of the image the pixel index runs over: n of the forward (OH x OW) and of
                               // the data gradient (H x W), k of the weight gradient (OH x OW)
    int st, pad;
    long long a_sm, a_sk;      // forward, data gradient: strides of w for the m channel and the reduction channel
    int chunks, S;             // chunks of CG_K in K; slices
    long long total;           // elements of the result: the pitch of a partial in the workspace
};

// x[b, c, h0 + r, w0 + s] with (h0, w0) = (oh st - p, ow st - p), 0 in the padding: no address is formed there
__device__ inline float cs_tap_x(const CsArgs& g, unsigned b, unsigned c, int h0, int w0, int r, int s, bool ok) {
    const int ih = h0 + r, iw = w0 + s;
    if (!ok || ih < 0 || ih >= g.BH || iw < 0 || iw >= g.BW) return 0.0f;
    return g.b[(((size_t)b * g.CR + c) * g.BH + ih) * g.BW + iw];
}

// t / st when t >= 0 and st divides it, else -1
__device__ inline int cs_exact(int t, int st) {
    if (t < 0) return -1;
    if (st == 1) return t;
    if (st == 2) return (t & 1) ? -1 : (t >> 1);
    const int q = t / st;
    return q * st == t ? q : -1;
}

// dy[b, c, (h0 - r) / st, (w0 - s) / st] with (h0, w0) = (ih + p, iw + p), 0 where a quotient is not exact or out of range
__device__ inline float cs_tap_dy(const CsArgs& g, unsigned b, unsigned c, int h0, int w0, int r, int s, bool ok) {
    if (!ok) return 0.0f;
    const int oh = cs_exact(h0 - r, g.st), ow = cs_exact(w0 - s, g.st);
    if (oh < 0 || oh >= g.BH || ow < 0 || ow >= g.BW) return 0.0f;
    return g.b[(((size_t)b * g.CR + c) * g.BH + oh) * g.BW + ow];
}

// forward and data gradient: A by (k fastest: 16 consecutive weights of a row forward), B by (pixel fastest: 64 consecutive
// pixels of a tap)
template <int R, int MODE>
struct CsDataMap {
    static constexpr bool B_K_FASTEST = false;
    static constexpr unsigned RR = R * R;
    unsigned ak, am0, bn, bk0, nb; int h0, w0; bool nok;
    __device__ inline CsDataMap(const CsArgs& g, unsigned m0, unsigned n0, int tid) {
        ak = tid & 15; am0 = m0 + (tid >> 4);
        bn = n0 + (tid & 63); bk0 = tid >> 6;
        nok = bn < g.N;
        nb = nok ? bn / g.PHW : 0;
        const unsigned hw = nok ? bn - nb * g.PHW : 0;
        const int nh = hw / g.PW, nw = hw - nh * g.PW;
        h0 = MODE == CS_FWD ? nh * g.st - g.pad : nh + g.pad;
        w0 = MODE == CS_FWD ? nw * g.st - g.pad : nw + g.pad;
    }
    __device__ inline void load(const CsArgs& g, unsigned chunk, CgStage& st) const {
        const unsigned k = chunk * CG_K + ak, kc = k / RR, rs = k - RR * kc;
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (k < g.K && m < g.M) ? g.a[(size_t)m * g.a_sm + (size_t)kc * g.a_sk + rs] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CG_PER; ++j) {
            const unsigned kb = chunk * CG_K + bk0 + 4 * j, c = kb / RR, t = kb - RR * c;
            const int r = t / R, s = t - R * r;
            const bool ok = nok && kb < g.K;
            st.b[j] = MODE == CS_FWD ? cs_tap_x(g, nb, c, h0, w0, r, s, ok) : cs_tap_dy(g, nb, c, h0, w0, r, s, ok);
        }
    }
};

// ---- the host side: sizes and the GEMM view of one product
struct CsDims { int B, Cin, Cout, H, W, R, st, pad, OH, OW; };

static int cs_dims(int B, int Cin, int Cout, int H, int W, int R, int st, int pad, CsDims* d) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    if ((R != 1 && R != 3 && R != 7) || st < 1 || pad < 0) return VPN_E_BADARG;
    const long long lim = 2147483647LL, Hp = (long long)H + 2LL * pad, Wp = (long long)W + 2LL * pad;
    if (Hp < R || Wp < R) return VPN_E_BADARG;
    if (Hp > lim || Wp > lim) return VPN_E_TOOBIG;                     // padded coordinates are ints
    const long long OH = (Hp - R) / st + 1, OW = (Wp - R) / st + 1, HW = (long long)H * W, OHW = OH * OW;
    if (HW > lim || HW * B > lim || HW * B * Cin > lim) return VPN_E_TOOBIG;
    if (OHW > lim || OHW * B > lim || OHW * B * Cout > lim) return VPN_E_TOOBIG;
    if ((long long)R * R * Cin * Cout > lim) return VPN_E_TOOBIG;
    d->B = B; d->Cin = Cin; d->Cout = Cout; d->H = H; d->W = W; d->R = R; d->st = st; d->pad = pad; d->OH = (int)OH; d->OW = (int)OW;
    return 0;
}

static int cs_plan(int product, const CsDims& d, CgPlan* p) {
    const unsigned RR = (unsigned)(d.R * d.R), P = (unsigned)d.B * d.OH * d.OW, Q = (unsigned)d.B * d.H * d.W;
    if (product == VPN_CONV_FWD) return cg_plan(d.Cout, P, RR * d.Cin, (long long)P * d.Cout, p);
    if (product == VPN_CONV_DX) return cg_plan(d.Cin, Q, RR * d.Cout, (long long)Q * d.Cin, p);
    if (product == VPN_CONV_DW) return cg_plan(d.Cout, RR * d.Cin, P, (long long)RR * d.Cin * d.Cout, p);
    return VPN_E_BADARG;
}

}  // namespace vpn
