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
//   * a workgroup of 256 (4 waves, 2 x 2) owns a 64 x 64 tile of D, every wave a 32 x 32 quarter in 16 accumulator
//     registers of v_mfma_f32_32x32x2_f32; K is walked in chunks of 16 through LDS ([k][m] and [k][n], so a wave reads its
//     operands along consecutive lanes), the next chunk's global loads are issued before the current chunk's MFMAs;
//   * padding, and the tails of all three GEMM dimensions, are masked loads: an address is formed only for an element that
//     exists, everything else enters the product as 0.0f;
//   * a call with fewer than VPN_CONV_SPLIT_TARGET tiles splits K over gridDim.z slices of whole chunks (balanced: slice z
//     owns the chunks [z n / S, (z + 1) n / S)); a slice writes its partial tile to the caller's workspace [S][D] and a second
//     launch adds the S partials of every element in the order 0 .. S - 1.  The host decides (cv_plan);
//   * one summation order: inside a slice the k-ordered fmaf chain of the MFMA, then the slices in order.  No atomics, no
//     grid barrier, nothing allocated, no host synchronisation: bit-equal from run to run and capturable;
//   * accesses: the operand loads are element loads, consecutive lanes on consecutive addresses (the shifted taps of a
//     row start at w - 1, w, w + 1: never all 16-byte aligned); the merge of the partials uses 16-byte accesses when the host
//     found the element count a multiple of 4 and the output 16-byte aligned, element accesses otherwise.
#include "vpn_common.h"
#include <type_traits>

namespace vpn {

constexpr int CV_T = VPN_CONV_TILE;          // rows and columns of D a workgroup owns
constexpr int CV_K = VPN_CONV_TILE_K;        // reduction elements per LDS chunk
constexpr int CV_BLOCK = 256;
constexpr int CV_LD = CV_T + 32;             // LDS row pitch: the two k rows a wave reads per MFMA land on disjoint banks
constexpr int CV_PER = CV_T * CV_K / CV_BLOCK;     // elements of each operand a work-item stages per chunk
static_assert(CV_T == 64 && CV_K == 16 && CV_PER == 4, "the staging maps below are written for 64 x 64 x 16 and 256 work-items");

#ifndef VPN_HOST_SHIM
typedef float f32x16 __attribute__((ext_vector_type(16)));
#endif

enum { CV_DATA = 0, CV_WGRAD = 1 };

struct CvArgs {
    const float* a;            // CV_DATA: the weights [C_out, C_in, 3, 3]; CV_WGRAD: dy [B, M, H, W]
    const float* b;            // CV_DATA: x (forward) or dy (data gradient) [B, CR, H, W]; CV_WGRAD: x [B, CR, H, W]
    float* out;                // the result, or the workspace [S][total] when S > 1
    unsigned M, N, K;          // the GEMM's sizes
    int CR;                    // channels of `b`: CV_DATA K = 9 CR, CV_WGRAD N = 9 CR
    int H, W, HW;
    long long a_sm, a_sk;      // CV_DATA: strides of w for the m channel and the reduction channel
    int flip;                  // CV_DATA: 1 mirrors the taps (data gradient)
    int chunks, S;             // chunks of CV_K in K; slices
    long long total;           // elements of the result: the pitch of a partial in the workspace
};

// what a work-item holds between the global loads of a chunk and its LDS stores
struct CvStage { float a[CV_PER], b[CV_PER]; };

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
    unsigned ak, am0, bn, bk0, nb; int nh, nw; bool nok;
    __device__ inline CvDataMap(const CvArgs& g, unsigned m0, unsigned n0, int tid) {
        ak = tid & 15; am0 = m0 + (tid >> 4);
        bn = n0 + (tid & 63); bk0 = tid >> 6;
        nok = bn < g.N;
        nb = nok ? bn / g.HW : 0;
        const unsigned hw = nok ? bn - nb * g.HW : 0;
        nh = hw / g.W; nw = hw - nh * g.W;
    }
    __device__ inline void load(const CvArgs& g, unsigned chunk, CvStage& st) const {
        const unsigned k = chunk * CV_K + ak, kc = k / 9, rs = k - 9 * kc;
#pragma unroll
        for (int j = 0; j < CV_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (k < g.K && m < g.M) ? g.a[(size_t)m * g.a_sm + (size_t)kc * g.a_sk + rs] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CV_PER; ++j) {
            const unsigned kb = chunk * CV_K + bk0 + 4 * j, c = kb / 9;
            int dh, dw;
            cv_tap(kb - 9 * c, g.flip, dh, dw);
            st.b[j] = cv_pixel(g.b, g, nb, c, nh, nw, dh, dw, nok && kb < g.K);
        }
    }
    __device__ inline void store(const CvStage& st, float (*As)[CV_LD], float (*Bs)[CV_LD], int tid) const {
#pragma unroll
        for (int j = 0; j < CV_PER; ++j) {
            As[tid & 15][(tid >> 4) + 16 * j] = st.a[j];
            Bs[(tid >> 6) + 4 * j][tid & 63] = st.b[j];
        }
    }
};

// CV_WGRAD: k is the pixel; both operands by (k fastest: 16 consecutive pixels of a channel)
struct CvWgradMap {
    unsigned kk, am0, bn0;
    __device__ inline CvWgradMap(const CvArgs&, unsigned m0, unsigned n0, int tid) {
        kk = tid & 15; am0 = m0 + (tid >> 4); bn0 = n0 + (tid >> 4);
    }
    __device__ inline void load(const CvArgs& g, unsigned chunk, CvStage& st) const {
        const unsigned p = chunk * CV_K + kk;
        const bool pok = p < g.K;
        const unsigned b = pok ? p / g.HW : 0, hw = pok ? p - b * g.HW : 0;
        const int h = hw / g.W, w = hw - h * g.W;
#pragma unroll
        for (int j = 0; j < CV_PER; ++j) {
            const unsigned m = am0 + 16 * j;
            st.a[j] = (pok && m < g.M) ? g.a[((size_t)b * g.M + m) * g.HW + hw] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < CV_PER; ++j) {
            const unsigned n = bn0 + 16 * j, c = n / 9;
            int dh, dw;
            cv_tap(n - 9 * c, 0, dh, dw);
            st.b[j] = cv_pixel(g.b, g, b, c, h, w, dh, dw, pok && n < g.N);
        }
    }
    __device__ inline void store(const CvStage& st, float (*As)[CV_LD], float (*Bs)[CV_LD], int tid) const {
#pragma unroll
        for (int j = 0; j < CV_PER; ++j) {
            As[tid & 15][(tid >> 4) + 16 * j] = st.a[j];
            Bs[tid & 15][(tid >> 4) + 16 * j] = st.b[j];
        }
    }
};

// grid (tiles of N, tiles of M, S)
template <int MODE>
__global__ __launch_bounds__(CV_BLOCK) void cv_gemm_kernel(CvArgs g) {
    __shared__ float As[CV_K][CV_LD];
    __shared__ float Bs[CV_K][CV_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n0 = blockIdx.x * CV_T, m0 = blockIdx.y * CV_T, z = blockIdx.z;
    if (m0 >= g.M || n0 >= g.N || z >= (unsigned)g.S) return;          // the host never asks
    const unsigned c0 = (unsigned)((unsigned long long)z * g.chunks / g.S);
    const unsigned c1 = (unsigned)((unsigned long long)(z + 1) * g.chunks / g.S);
    typename std::conditional<MODE == CV_DATA, CvDataMap, CvWgradMap>::type map(g, m0, n0, tid);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, col = lane & 31, half = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    CvStage st;
    if (c0 < c1) map.load(g, c0, st);
    for (unsigned c = c0; c < c1; ++c) {
        __syncthreads();                                     // the previous chunk has been read by every wave
        map.store(st, As, Bs, tid);
        __syncthreads();
        if (c + 1 < c1) map.load(g, c + 1, st);
#pragma unroll
        for (int t = 0; t < CV_K / 2; ++t)                   // lane: A[row col][k half], B[k half][column col]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * t + half][wm + col], Bs[2 * t + half][wn + col], acc, 0, 0, 0);
    }
    // D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const unsigned n = n0 + wn + col;
    if (n >= g.N) return;
    float* out = g.out + (size_t)z * g.total;
    size_t base, pitch;
    if (MODE == CV_DATA) {
        const unsigned b = n / g.HW;
        base = (size_t)b * g.M * g.HW + (n - b * g.HW); pitch = g.HW;
    } else {
        base = n; pitch = g.N;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < g.M) out[base + (size_t)m * pitch] = acc[r];
    }
}

template <int V> struct CvVec { float v[V]; };
template <int V> __device__ inline CvVec<V> cv_ldv(const float* p);
template <> __device__ inline CvVec<1> cv_ldv<1>(const float* p) { CvVec<1> r; r.v[0] = p[0]; return r; }
template <> __device__ inline CvVec<4> cv_ldv<4>(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    CvVec<4> r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r;
}
template <int V> __device__ inline void cv_stv(float* p, const CvVec<V>& r);
template <> __device__ inline void cv_stv<1>(float* p, const CvVec<1>& r) { p[0] = r.v[0]; }
template <> __device__ inline void cv_stv<4>(float* p, const CvVec<4>& r) {
    float4 q; q.x = r.v[0]; q.y = r.v[1]; q.z = r.v[2]; q.w = r.v[3];
    *reinterpret_cast<float4*>(p) = q;
}

// out[i] = ws[0][i] + ws[1][i] + ... + ws[S - 1][i], in that order; `units` accesses of V floats
template <int V>
__global__ __launch_bounds__(CV_BLOCK) void cv_merge_kernel(const float* ws, float* out, long long units, long long total, int S) {
    const long long u = (long long)blockIdx.x * CV_BLOCK + threadIdx.x;
    if (u >= units) return;
    CvVec<V> r = cv_ldv<V>(ws + u * V);
    for (int s = 1; s < S; ++s) {
        const CvVec<V> q = cv_ldv<V>(ws + (size_t)s * total + u * V);
#pragma unroll
        for (int j = 0; j < V; ++j) r.v[j] += q.v[j];
    }
    cv_stv<V>(out + u * V, r);
}

// ---- the host rule: sizes, tiles and slices of one product
struct CvPlan { unsigned M, N, K; int CR, chunks, S; unsigned mt, nt; long long total; };

static int cv_sizes(int B, int Cin, int Cout, int H, int W) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    const long long HW = (long long)H * W, lim = 2147483647LL;
    if (HW > lim || HW * B > lim || HW * B * Cin > lim || HW * B * Cout > lim || 9LL * Cin * Cout > lim) return VPN_E_TOOBIG;
    return 0;
}

static int cv_plan(int product, int B, int Cin, int Cout, int H, int W, CvPlan* p) {
    const int rc = cv_sizes(B, Cin, Cout, H, W);
    if (rc) return rc;
    const unsigned P = (unsigned)B * H * W;
    if (product == VPN_CONV_FWD) { p->M = Cout; p->N = P; p->K = 9u * Cin; p->CR = Cin; p->total = (long long)P * Cout; }
    else if (product == VPN_CONV_DX) { p->M = Cin; p->N = P; p->K = 9u * Cout; p->CR = Cout; p->total = (long long)P * Cin; }
    else if (product == VPN_CONV_DW) { p->M = Cout; p->N = 9u * Cin; p->K = P; p->CR = Cin; p->total = 9LL * Cin * Cout; }
    else return VPN_E_BADARG;
    p->mt = (p->M + CV_T - 1) / CV_T;
    p->nt = (unsigned)(((unsigned long long)p->N + CV_T - 1) / CV_T);
    if (p->mt > 65535u) return VPN_E_TOOBIG;                         // gridDim.y
    p->chunks = (int)(((unsigned long long)p->K + CV_K - 1) / CV_K);
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

static size_t cv_ws_bytes(const CvPlan& p) { return p.S > 1 ? (size_t)p.S * (size_t)p.total * sizeof(float) : 0; }

static int cv_run(int product, const CvPlan& p, const float* a, const float* b, float* out, int Cin, int H, int W, void* ws, hipStream_t st) {
    CvArgs g;
    g.a = a; g.b = b; g.out = p.S > 1 ? (float*)ws : out;
    g.M = p.M; g.N = p.N; g.K = p.K; g.CR = p.CR; g.H = H; g.W = W; g.HW = H * W;
    g.a_sm = product == VPN_CONV_FWD ? 9LL * Cin : 9; g.a_sk = product == VPN_CONV_FWD ? 9 : 9LL * Cin;
    g.flip = product == VPN_CONV_DX; g.chunks = p.chunks; g.S = p.S; g.total = p.total;
    const dim3 grid(p.nt, p.mt, (unsigned)p.S);
    if (product == VPN_CONV_DW) VPN_LAUNCH_AS("cv_gemm_kernel<wgrad>", (cv_gemm_kernel<CV_WGRAD>), grid, dim3(CV_BLOCK), 0, st, g);
    else VPN_LAUNCH_AS("cv_gemm_kernel<data>", (cv_gemm_kernel<CV_DATA>), grid, dim3(CV_BLOCK), 0, st, g);
    VPN_LAUNCH_CHECK();
    if (p.S > 1) {
        const bool vec = p.total % 4 == 0 && ((uintptr_t)out & 15) == 0;          // the workspace is 16-byte aligned (checked)
        const long long units = vec ? p.total / 4 : p.total;
        const dim3 mg((unsigned)((units + CV_BLOCK - 1) / CV_BLOCK));
        if (vec) VPN_LAUNCH_AS("cv_merge_kernel", (cv_merge_kernel<4>), mg, dim3(CV_BLOCK), 0, st, (const float*)ws, out, units, p.total, p.S);
        else VPN_LAUNCH_AS("cv_merge_kernel", (cv_merge_kernel<1>), mg, dim3(CV_BLOCK), 0, st, (const float*)ws, out, units, p.total, p.S);
        VPN_LAUNCH_CHECK();
    }
    return 0;
}

static bool cv_ws_bad(size_t need, const void* ws, size_t bytes) { return need && (!ws || bytes < need || ((uintptr_t)ws & 15)); }

}  // namespace vpn

using namespace vpn;

extern "C" int vpn_conv3x3_splits(int B, int C_in, int C_out, int H, int W, int product) {
    CvPlan p;
    const int rc = cv_plan(product, B, C_in, C_out, H, W, &p);
    return rc ? rc : p.S;
}

extern "C" size_t vpn_conv3x3_workspace(int B, int C_in, int C_out, int H, int W, int products) {
    size_t need = 0;
    for (int product : {VPN_CONV_FWD, VPN_CONV_DX, VPN_CONV_DW}) {
        CvPlan p;
        if (!(products & product)) continue;
        if (cv_plan(product, B, C_in, C_out, H, W, &p) != 0) return 0;
        if (cv_ws_bytes(p) > need) need = cv_ws_bytes(p);
    }
    return need;
}

extern "C" int vpn_conv3x3_fwd(const float* x, const float* w, float* y, int B, int C_in, int C_out, int H, int W, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return VPN_E_BADARG;
    CvPlan p;
    const int rc = cv_plan(VPN_CONV_FWD, B, C_in, C_out, H, W, &p);
    if (rc) return rc;
    if (cv_ws_bad(cv_ws_bytes(p), workspace, workspace_bytes)) return VPN_E_BADARG;
    return cv_run(VPN_CONV_FWD, p, w, x, y, C_in, H, W, workspace, (hipStream_t)stream);
}

extern "C" int vpn_conv3x3_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int C_in, int C_out, int H,
                               int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !w) return VPN_E_BADARG;
    CvPlan pd, pw;
    int rc = cv_plan(VPN_CONV_DX, B, C_in, C_out, H, W, &pd);
    if (!rc) rc = cv_plan(VPN_CONV_DW, B, C_in, C_out, H, W, &pw);
    if (rc) return rc;
    if ((dx && cv_ws_bad(cv_ws_bytes(pd), workspace, workspace_bytes)) || (dw && cv_ws_bad(cv_ws_bytes(pw), workspace, workspace_bytes)))
        return VPN_E_BADARG;
    // the two products use the workspace one after the other: launches of one stream run in order
    if (dx) { rc = cv_run(VPN_CONV_DX, pd, w, dy, dx, C_in, H, W, workspace, (hipStream_t)stream); if (rc) return rc; }
    if (dw) { rc = cv_run(VPN_CONV_DW, pw, dy, x, dw, C_in, H, W, workspace, (hipStream_t)stream); if (rc) return rc; }
    return 0;
}
