// trunkstride.hip — the trunk's remaining convolutions (gfx950): square kernel R in {1, 3, 7}, any stride >= 1, any padding
// >= 0, dilation 1, groups 1, no bias, as an implicit GEMM on the f32-input MFMA, forward, data gradient and weight gradient
// (DESIGN.md 4.20).  The scheme is trunkconv.hip's, generalised; nothing here is a second design.
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
//   * a workgroup of 256 (4 waves, 2 x 2) owns a 64 x 64 tile of D, every wave a 32 x 32 quarter in 16 accumulator
//     registers of v_mfma_f32_32x32x2_f32; K is walked in chunks of 16 through LDS ([k][m] and [k][n]), the next chunk's
//     global loads are issued before the current chunk's MFMAs;
//   * padding, stride gaps and the tails of all three GEMM dimensions are masked loads: an address is formed only for an
//     element that exists, everything else enters the product as 0.0f;
//   * the split rule is trunkconv.hip's over the generalised M, N, K with the same VPN_CONV_* constants: fewer than
//     VPN_CONV_SPLIT_TARGET tiles split K over gridDim.z slices of whole chunks (slice z owns the chunks
//     [z n / S, (z + 1) n / S)), the partial tiles go to the caller's workspace [S][D] and a second launch adds them in the
//     order 0 .. S - 1;
//   * one summation order: inside a slice the k-ordered fmaf chain of the MFMA, then the slices in order.  No atomics, no
//     grid barrier, nothing allocated, no host synchronisation: bit-equal from run to run and capturable.  For R = 3,
//     stride 1, padding 1 the order is trunkconv.hip's: the results are bit-equal to vpn_conv3x3_*.
// The tile loop, the epilogue, the merge and the plan are this file's own copy of trunkconv.hip's (names cs_*): that file
// is held to exactly four kernels and stays untouched.
#include "vpn_common.h"

namespace vpn {

constexpr int CS_T = VPN_CONV_TILE;          // rows and columns of D a workgroup owns
constexpr int CS_K = VPN_CONV_TILE_K;        // reduction elements per LDS chunk
constexpr int CS_BLOCK = 256;
constexpr int CS_LD = CS_T + 32;             // LDS row pitch: the two k rows a wave reads per MFMA land on disjoint banks
constexpr int CS_PER = CS_T * CS_K / CS_BLOCK;     // elements of each operand a work-item stages per chunk
static_assert(CS_T == 64 && CS_K == 16 && CS_PER == 4, "the staging maps below are written for 64 x 64 x 16 and 256 work-items");

#ifndef VPN_HOST_SHIM
typedef float cs_f32x16 __attribute__((ext_vector_type(16)));
#else
typedef f32x16 cs_f32x16;
#endif

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
    int chunks, S;             // chunks of CS_K in K; slices
    long long total;           // elements of the result: the pitch of a partial in the workspace
};

// what a work-item holds between the global loads of a chunk and its LDS stores
struct CsStage { float a[CS_PER], b[CS_PER]; };

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
    __device__ inline void load(const CsArgs& g, unsigned chunk, CsStage& st) const {
        const unsigned k = chunk * CS_K + ak, kc = k / RR, rs = k - RR * kc;
#pragma unroll
        for (int j = 0; j < CS_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (k < g.K && m < g.M) ? g.a[(size_t)m * g.a_sm + (size_t)kc * g.a_sk + rs] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CS_PER; ++j) {
            const unsigned kb = chunk * CS_K + bk0 + 4 * j, c = kb / RR, t = kb - RR * c;
            const int r = t / R, s = t - R * r;
            const bool ok = nok && kb < g.K;
            st.b[j] = MODE == CS_FWD ? cs_tap_x(g, nb, c, h0, w0, r, s, ok) : cs_tap_dy(g, nb, c, h0, w0, r, s, ok);
        }
    }
    __device__ inline void store(const CsStage& st, float (*As)[CS_LD], float (*Bs)[CS_LD], int tid) const {
#pragma unroll
        for (int j = 0; j < CS_PER; ++j) {
            As[tid & 15][(tid >> 4) + 16 * j] = st.a[j];
            Bs[(tid >> 6) + 4 * j][tid & 63] = st.b[j];
        }
    }
};

// weight gradient: k is the output pixel; both operands by (k fastest: 16 consecutive pixels of a channel)
template <int R>
struct CsWgradMap {
    static constexpr unsigned RR = R * R;
    unsigned kk, am0, bn0;
    __device__ inline CsWgradMap(const CsArgs&, unsigned m0, unsigned n0, int tid) {
        kk = tid & 15; am0 = m0 + (tid >> 4); bn0 = n0 + (tid >> 4);
    }
    __device__ inline void load(const CsArgs& g, unsigned chunk, CsStage& st) const {
        const unsigned p = chunk * CS_K + kk;
        const bool pok = p < g.K;
        const unsigned b = pok ? p / g.PHW : 0, hw = pok ? p - b * g.PHW : 0;
        const int oh = hw / g.PW, ow = hw - oh * g.PW;
        const int h0 = oh * g.st - g.pad, w0 = ow * g.st - g.pad;
#pragma unroll
        for (int j = 0; j < CS_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (pok && m < g.M) ? g.a[((size_t)b * g.M + m) * g.PHW + hw] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CS_PER; ++j) {
            const unsigned n = bn0 + 16 * j, c = n / RR, t = n - RR * c;
            const int r = t / R, s = t - R * r;
            st.b[j] = cs_tap_x(g, b, c, h0, w0, r, s, pok && n < g.N);
        }
    }
    __device__ inline void store(const CsStage& st, float (*As)[CS_LD], float (*Bs)[CS_LD], int tid) const {
#pragma unroll
        for (int j = 0; j < CS_PER; ++j) {
            As[tid & 15][(tid >> 4) + 16 * j] = st.a[j];
            Bs[tid & 15][(tid >> 4) + 16 * j] = st.b[j];
        }
    }
};

template <int R, int MODE> struct CsMapOf { typedef CsDataMap<R, MODE> type; };
template <int R> struct CsMapOf<R, CS_DW> { typedef CsWgradMap<R> type; };

// grid (tiles of N, tiles of M, S)
template <int R, int MODE>
__global__ __launch_bounds__(CS_BLOCK) void cs_gemm_kernel(CsArgs g) {
    __shared__ float As[CS_K][CS_LD];
    __shared__ float Bs[CS_K][CS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n0 = blockIdx.x * CS_T, m0 = blockIdx.y * CS_T, z = blockIdx.z;
    if (m0 >= g.M || n0 >= g.N || z >= (unsigned)g.S) return;          // the host never asks
    const unsigned c0 = (unsigned)((unsigned long long)z * g.chunks / g.S);
    const unsigned c1 = (unsigned)((unsigned long long)(z + 1) * g.chunks / g.S);
    typename CsMapOf<R, MODE>::type map(g, m0, n0, tid);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, col = lane & 31, half = lane >> 5;
    cs_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    CsStage st;
    if (c0 < c1) map.load(g, c0, st);
    for (unsigned c = c0; c < c1; ++c) {
        __syncthreads();                                     // the previous chunk has been read by every wave
        map.store(st, As, Bs, tid);
        __syncthreads();
        if (c + 1 < c1) map.load(g, c + 1, st);
#pragma unroll
        for (int t = 0; t < CS_K / 2; ++t)                   // lane: A[row col][k half], B[k half][column col]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * t + half][wm + col], Bs[2 * t + half][wn + col], acc, 0, 0, 0);
    }
    // D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const unsigned n = n0 + wn + col;
    if (n >= g.N) return;
    float* out = g.out + (size_t)z * g.total;
    size_t base, pitch;
    if (MODE != CS_DW) {
        const unsigned b = n / g.PHW;
        base = (size_t)b * g.M * g.PHW + (n - b * g.PHW); pitch = g.PHW;
    } else {
        base = n; pitch = g.N;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < g.M) out[base + (size_t)m * pitch] = acc[r];
    }
}

template <int V> struct CsVec { float v[V]; };
template <int V> __device__ inline CsVec<V> cs_ldv(const float* p);
template <> __device__ inline CsVec<1> cs_ldv<1>(const float* p) { CsVec<1> r; r.v[0] = p[0]; return r; }
template <> __device__ inline CsVec<4> cs_ldv<4>(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    CsVec<4> r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r;
}
template <int V> __device__ inline void cs_stv(float* p, const CsVec<V>& r);
template <> __device__ inline void cs_stv<1>(float* p, const CsVec<1>& r) { p[0] = r.v[0]; }
template <> __device__ inline void cs_stv<4>(float* p, const CsVec<4>& r) {
    float4 q; q.x = r.v[0]; q.y = r.v[1]; q.z = r.v[2]; q.w = r.v[3];
    *reinterpret_cast<float4*>(p) = q;
}

// out[i] = ws[0][i] + ws[1][i] + ... + ws[S - 1][i], in that order; `units` accesses of V floats
template <int V>
__global__ __launch_bounds__(CS_BLOCK) void cs_merge_kernel(const float* ws, float* out, long long units, long long total, int S) {
    const long long u = (long long)blockIdx.x * CS_BLOCK + threadIdx.x;
    if (u >= units) return;
    CsVec<V> r = cs_ldv<V>(ws + u * V);
    for (int s = 1; s < S; ++s) {
        const CsVec<V> q = cs_ldv<V>(ws + (size_t)s * total + u * V);
#pragma unroll
        for (int j = 0; j < V; ++j) r.v[j] += q.v[j];
    }
    cs_stv<V>(out + u * V, r);
}

// ---- the host rule: sizes, tiles and slices of one product
struct CsDims { int B, Cin, Cout, H, W, R, st, pad, OH, OW; };
struct CsPlan { unsigned M, N, K; int chunks, S; unsigned mt, nt; long long total; };

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

static int cs_plan(int product, const CsDims& d, CsPlan* p) {
    const unsigned RR = (unsigned)(d.R * d.R), P = (unsigned)d.B * d.OH * d.OW, Q = (unsigned)d.B * d.H * d.W;
    if (product == VPN_CONV_FWD) { p->M = d.Cout; p->N = P; p->K = RR * d.Cin; p->total = (long long)P * d.Cout; }
    else if (product == VPN_CONV_DX) { p->M = d.Cin; p->N = Q; p->K = RR * d.Cout; p->total = (long long)Q * d.Cin; }
    else if (product == VPN_CONV_DW) { p->M = d.Cout; p->N = RR * d.Cin; p->K = P; p->total = (long long)RR * d.Cin * d.Cout; }
    else return VPN_E_BADARG;
    p->mt = (p->M + CS_T - 1) / CS_T;
    p->nt = (unsigned)(((unsigned long long)p->N + CS_T - 1) / CS_T);
    if (p->mt > 65535u) return VPN_E_TOOBIG;                         // gridDim.y
    p->chunks = (int)(((unsigned long long)p->K + CS_K - 1) / CS_K);
    const unsigned long long tiles = (unsigned long long)p->mt * p->nt;
    long long S = 1;
    if (tiles < VPN_CONV_SPLIT_TARGET) {
        S = (long long)((VPN_CONV_SPLIT_TARGET + tiles - 1) / tiles);
        if (S > VPN_CONV_MAX_SPLIT) S = VPN_CONV_MAX_SPLIT;
        if (S > p->chunks) S = p->chunks;
    }
    p->S = (int)S;
    return 0;
}

static size_t cs_ws_bytes(const CsPlan& p) { return p.S > 1 ? (size_t)p.S * (size_t)p.total * sizeof(float) : 0; }

template <int R>
static void cs_launch(int product, const dim3& grid, hipStream_t st, const CsArgs& g) {
    if (product == VPN_CONV_FWD) VPN_LAUNCH_AS("cs_gemm_kernel<fwd>", (cs_gemm_kernel<R, CS_FWD>), grid, dim3(CS_BLOCK), 0, st, g);
    else if (product == VPN_CONV_DX) VPN_LAUNCH_AS("cs_gemm_kernel<dx>", (cs_gemm_kernel<R, CS_DX>), grid, dim3(CS_BLOCK), 0, st, g);
    else VPN_LAUNCH_AS("cs_gemm_kernel<dw>", (cs_gemm_kernel<R, CS_DW>), grid, dim3(CS_BLOCK), 0, st, g);
}

static int cs_run(int product, const CsDims& d, const CsPlan& p, const float* a, const float* b, float* out, void* ws, hipStream_t st) {
    const long long RR = (long long)d.R * d.R;
    CsArgs g;
    g.a = a; g.b = b; g.out = p.S > 1 ? (float*)ws : out;
    g.M = p.M; g.N = p.N; g.K = p.K;
    g.CR = product == VPN_CONV_DX ? d.Cout : d.Cin;
    g.BH = product == VPN_CONV_DX ? d.OH : d.H; g.BW = product == VPN_CONV_DX ? d.OW : d.W;
    g.PW = product == VPN_CONV_DX ? d.W : d.OW; g.PHW = (product == VPN_CONV_DX ? d.H : d.OH) * g.PW;
    g.st = d.st; g.pad = d.pad;
    g.a_sm = product == VPN_CONV_FWD ? RR * d.Cin : RR; g.a_sk = product == VPN_CONV_FWD ? RR : RR * d.Cin;
    g.chunks = p.chunks; g.S = p.S; g.total = p.total;
    const dim3 grid(p.nt, p.mt, (unsigned)p.S);
    if (d.R == 1) cs_launch<1>(product, grid, st, g);
    else if (d.R == 3) cs_launch<3>(product, grid, st, g);
    else cs_launch<7>(product, grid, st, g);
    VPN_LAUNCH_CHECK();
    if (p.S > 1) {
        const bool vec = p.total % 4 == 0 && ((uintptr_t)out & 15) == 0;          // the workspace is 16-byte aligned (checked)
        const long long units = vec ? p.total / 4 : p.total;
        const dim3 mg((unsigned)((units + CS_BLOCK - 1) / CS_BLOCK));
        if (vec) VPN_LAUNCH_AS("cs_merge_kernel", (cs_merge_kernel<4>), mg, dim3(CS_BLOCK), 0, st, (const float*)ws, out, units, p.total, p.S);
        else VPN_LAUNCH_AS("cs_merge_kernel", (cs_merge_kernel<1>), mg, dim3(CS_BLOCK), 0, st, (const float*)ws, out, units, p.total, p.S);
        VPN_LAUNCH_CHECK();
    }
    return 0;
}

static bool cs_ws_bad(size_t need, const void* ws, size_t bytes) { return need && (!ws || bytes < need || ((uintptr_t)ws & 15)); }

}  // namespace vpn

using namespace vpn;

extern "C" int vpn_conv2d_splits(int B, int C_in, int C_out, int H, int W, int R, int stride, int pad, int product) {
    CsDims d;
    CsPlan p;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(product, d, &p);
    return rc ? rc : p.S;
}

extern "C" size_t vpn_conv2d_workspace(int B, int C_in, int C_out, int H, int W, int R, int stride, int pad, int products) {
    CsDims d;
    if (cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d) != 0) return 0;
    size_t need = 0;
    for (int product : {VPN_CONV_FWD, VPN_CONV_DX, VPN_CONV_DW}) {
        CsPlan p;
        if (!(products & product)) continue;
        if (cs_plan(product, d, &p) != 0) return 0;
        if (cs_ws_bytes(p) > need) need = cs_ws_bytes(p);
    }
    return need;
}

extern "C" int vpn_conv2d_fwd(const float* x, const float* w, float* y, int B, int C_in, int C_out, int H, int W, int R, int stride,
                              int pad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return VPN_E_BADARG;
    CsDims d;
    CsPlan p;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(VPN_CONV_FWD, d, &p);
    if (rc) return rc;
    if (cs_ws_bad(cs_ws_bytes(p), workspace, workspace_bytes)) return VPN_E_BADARG;
    return cs_run(VPN_CONV_FWD, d, p, w, x, y, workspace, (hipStream_t)stream);
}

extern "C" int vpn_conv2d_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int C_in, int C_out, int H,
                              int W, int R, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !w) return VPN_E_BADARG;
    CsDims d;
    CsPlan pd, pw;
    int rc = cs_dims(B, C_in, C_out, H, W, R, stride, pad, &d);
    if (!rc) rc = cs_plan(VPN_CONV_DX, d, &pd);
    if (!rc) rc = cs_plan(VPN_CONV_DW, d, &pw);
    if (rc) return rc;
    if ((dx && cs_ws_bad(cs_ws_bytes(pd), workspace, workspace_bytes)) || (dw && cs_ws_bad(cs_ws_bytes(pw), workspace, workspace_bytes)))
        return VPN_E_BADARG;
    // the two products use the workspace one after the other: launches of one stream run in order
    if (dx) { rc = cs_run(VPN_CONV_DX, d, pd, w, dy, dx, workspace, (hipStream_t)stream); if (rc) return rc; }
    if (dw) { rc = cs_run(VPN_CONV_DW, d, pw, dy, x, dw, workspace, (hipStream_t)stream); if (rc) return rc; }
    return 0;
}
