// trunknorm.hip — the trunk's norm / add / ReLU ring (gfx950): batch norm, the residual add and the ReLU of a ResNet-18
// site as ONE op, forward and backward, the stem's form of it that also holds the 3x3 stride-2 max
// pool (the tp_ kernels below) and the tail's form that also holds the global average pool (DESIGN.md
// 4.22; the tt_ kernels below).
//
// Replaces, around the convolutions of the reference's torchvision trunk (vpnet_one_resnet.py:21, vpnet_two_resnet.py:21-22,
// sdnet.py:13), `relu(bn1(.))`, `bn2(.)`, `out += identity; relu(out)` and the downsample branch's norm: 20 training-mode
// batch norms, 17 ReLUs and 8 adds, each its own ATen kernel forward and again backward.  NCHW contiguous, fp32.
//   * statistics by an exact-mean second pass over values kept on chip (LDS in the one-pass regime, registers in a slice of
//     the split regime), slices merged by Chan's (count, mean, M2) rule around their exact mean: never E[x^2] - E[x]^2;
//   * two regimes chosen on the host from N = B H W.  N <= VPN_BN_ONE_PASS_MAX: one workgroup owns a channel, its slab
//     stays in LDS between the statistics and the normalisation, ONE launch, x read once.  Larger N: grid (C, S) with S
//     slices of VPN_BN_SLICE elements per channel; launch 1 writes per-slice partials, in launch 2 the first wave of every
//     workgroup of a channel merges the S partials in the same order (the same value everywhere: no atomics, no grid
//     barrier) and the workgroup normalises its slice;
//   * an element is addressed as (channel, batch row, offset): one division per work-item, then additions; 16-byte accesses
//     where the host found H W a multiple of 4 and every pointer 16-byte aligned, element accesses with the same indexing
//     otherwise;
//   * one summation order (per work-item in index order, then the wave's butterfly, then the waves in order; the
//     slices lane-strided, then the butterfly): bit-equal from run to run; no float atomics, no host synchronisation, nothing allocated;
//   * save_mean / save_invstd, the running statistics and the int64 batch counter are written by ONE work-item per channel
//     of the launch that knows the statistics.
// The three forms share their pieces.  Forward: tn_slab_stats / tn_stats_kernel, the apply kernels' statistics prelude
// (tn_apply_stats), the activation (tn_act) and the norm + residual + ReLU of a unit (tn_unit); what a form does with a unit
// afterwards (store, pool window, row mean) is its own kernel: tn_fwd_*, tp_fwd_*, tt_fwd_*.  Backward: ONE set of kernels,
// bwd_onepass_kernel / bwd_partial_kernel / bwd_apply_kernel, over a gradient source (ActGrad, TailGrad, PoolGrad) that
// says how a unit's upstream gradient and xhat are loaded and whether the form has a d_residual.  Host: tn_fwd_plan and
// tn_bwd hold the checks and the regime rules of all six entry points, tn_pick the <BLOCK, V> ladders.  The launch
// labels keep the forms' names: tn_*, tp_*, tt_*.
#include "vpn_common.h"
#include <type_traits>

namespace vpn {

constexpr int TN_MAX = VPN_BN_ONE_PASS_MAX;     // floats of a channel's slab held in LDS by the one-pass kernels
constexpr int TN_SLICE = VPN_BN_SLICE;          // elements of a slice of the split regime
constexpr int TN_BLOCK = 256;
constexpr int TN_PER = TN_SLICE / TN_BLOCK;     // elements a work-item holds in registers in tn_stats_kernel
constexpr int TN_SMALL = 512;                   // N up to here: one wave owns the channel
static_assert(TN_PER * TN_BLOCK == TN_SLICE && TN_PER % 4 == 0 && TN_MAX % 4 == 0 && TN_SMALL % 4 == 0 && TN_SMALL <= TN_MAX, "a slice is TN_PER elements per work-item");

// N = B HW elements per channel; in units of V floats (V = 4: 16-byte accesses, V = 1: elements): RU units per batch row,
// NU units per channel; step_b / step_i: the block size in units as (rows, units) = divmod(block, RU), formed on the host
struct TnShape { int C, HW, N, RU, NU, step_b, step_i, S; };

struct TnFwd {
    const float *x, *res, *w, *b;
    float *rm, *rv; long long* nbt;
    float *y, *save_mean, *save_invstd;
    float* ws;                     // split regime: [C, S, 2] (mean, M2) of every slice; NULL in tn_fwd_apply_kernel: eval
    float momentum, eps; int relu;
};

struct TnBwd {
    const float *dy, *x, *y, *w, *stat_a, *stat_b;       // y: NULL without ReLU; stat_b: invstd, or the running variance (eval)
    float *dx, *dres, *dw, *db;                          // each may be NULL: not wanted
    float* ws;                                           // split regime: [C, S, 2] (sum g, sum g xhat) of every slice
    float eps; int eval, sums;                           // sums: the apply kernel merges the partials
};

template <int V> struct Vec { float v[V]; };
template <int V> __device__ inline Vec<V> ldv(const float* p);
template <> __device__ inline Vec<1> ldv<1>(const float* p) { Vec<1> r; r.v[0] = p[0]; return r; }
template <> __device__ inline Vec<4> ldv<4>(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    Vec<4> r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r;
}
template <int V> __device__ inline void stv(float* p, const Vec<V>& r);
template <> __device__ inline void stv<1>(float* p, const Vec<1>& r) { p[0] = r.v[0]; }
template <> __device__ inline void stv<4>(float* p, const Vec<4>& r) {
    float4 q; q.x = r.v[0]; q.y = r.v[1]; q.z = r.v[2]; q.w = r.v[3];
    *reinterpret_cast<float4*>(p) = q;
}

// (batch row, unit in the row) of a unit of a channel, advanced by a fixed stride without a division
struct TnWalk {
    int b, i;
    __device__ inline TnWalk(int u, int RU) { b = u / RU; i = u - b * RU; }
    __device__ inline void step(const TnShape& s) { b += s.step_b; i += s.step_i; if (i >= s.RU) { i -= s.RU; ++b; } }
    template <int V> __device__ inline size_t at(const TnShape& s) const { return (size_t)b * s.C * s.HW + (size_t)i * V; }
};

// the sums of a and b over the workgroup, in every work-item: butterfly in the wave, then the waves in order
template <int BLOCK> __device__ inline void block_sum2(float& a, float& b, float* red) {
    a = wave_sum(a); b = wave_sum(b);
    if (BLOCK > 64) {
        const int w = threadIdx.x >> 6;
        __syncthreads();                      // the previous reduction's values have been read
        if ((threadIdx.x & 63) == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
        __syncthreads();
        a = 0.0f; b = 0.0f;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) { a += red[2 * i]; b += red[2 * i + 1]; }
    }
}

__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// what one work-item per channel writes once the statistics are known
__device__ inline void tn_publish(const TnFwd& a, int c, int N, float mean, float var, float invstd) {
    a.save_mean[c] = mean;
    a.save_invstd[c] = invstd;
    if (a.rm) a.rm[c] = (1.0f - a.momentum) * a.rm[c] + a.momentum * mean;
    if (a.rv) a.rv[c] = (1.0f - a.momentum) * a.rv[c] + a.momentum * (var * ((float)N / (float)(N - 1)));
    if (a.nbt && c == 0) a.nbt[0] += 1;
}

// the activation of all three forms, its roundings pinned: the product with gamma and the sum with beta are one fma
__device__ inline float tn_act(float x, float mean, float invstd, float gamma, float beta) {
    return __builtin_fmaf((x - mean) * invstd, gamma, beta);
}

// norm + residual + ReLU of the unit at element e, on its V values r in place
template <int V>
__device__ inline void tn_unit(const TnFwd& a, size_t e, Vec<V>& r, float mean, float invstd, float gamma, float beta) {
    Vec<V> q = {};
    if (a.res) q = ldv<V>(a.res + e);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float y = tn_act(r.v[j], mean, invstd, gamma, beta);
        if (a.res) y += q.v[j];
        r.v[j] = a.relu ? fmaxf(y, 0.0f) : y;
    }
}

// the statistics of a channel whose slab fits LDS (xc: the channel's first element): the slab filled in unit order, then
// the mean, the biased variance and invstd, the same in every work-item
template <int BLOCK, int V>
__device__ inline void tn_slab_stats(const TnShape& s, const float* xc, float eps, float* slab, float* red, float& mean, float& var,
                                     float& invstd) {
    const int tid = threadIdx.x;
    float sum = 0.0f, m2 = 0.0f;
    {
        TnWalk k(tid, s.RU);
        for (int u = tid; u < s.NU; u += BLOCK, k.step(s)) {
            const Vec<V> r = ldv<V>(xc + k.at<V>(s));
            stv<V>(slab + (size_t)u * V, r);
#pragma unroll
            for (int j = 0; j < V; ++j) sum += r.v[j];
        }
    }
    block_sum2<BLOCK>(sum, m2, red);
    // second pass around the first mean: the sum of the differences corrects the mean's own rounding (and M2 with it)
    const float mean0 = sum / (float)s.N;
    float rs = 0.0f;
    m2 = 0.0f;
    for (int u = tid; u < s.NU; u += BLOCK) {
        const Vec<V> r = ldv<V>(slab + (size_t)u * V);
#pragma unroll
        for (int j = 0; j < V; ++j) { const float d = r.v[j] - mean0; rs += d; m2 += d * d; }
    }
    block_sum2<BLOCK>(rs, m2, red);
    const float dm = rs / (float)s.N;
    mean = mean0 + dm;
    var = fmaxf(m2 - rs * dm, 0.0f) / (float)s.N;
    invstd = 1.0f / sqrtf(var + eps);
}

// ---- forward, one-pass regime: grid C, one workgroup (BLOCK = 64: one wave) per channel.  A work-item reads back from
// LDS only what it wrote itself, so the slab needs no barrier.
template <int BLOCK, int V>
__global__ __launch_bounds__(BLOCK) void tn_fwd_onepass_kernel(TnShape s, TnFwd a) {
    constexpr int SLAB = BLOCK == 64 ? TN_SMALL : TN_MAX;      // the one-wave form leaves the CU's LDS to other workgroups
    __shared__ __attribute__((aligned(16))) float slab[SLAB];
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (s.N > SLAB) return;                         // the host never asks: nothing outside the slab either way
    const size_t chan = (size_t)c * s.HW;
    float mean, var, invstd;
    tn_slab_stats<BLOCK, V>(s, a.x + chan, a.eps, slab, red, mean, var, invstd);
    if (tid == 0) tn_publish(a, c, s.N, mean, var, invstd);
    const float gamma = a.w ? a.w[c] : 1.0f, beta = a.b ? a.b[c] : 0.0f;
    TnWalk k(tid, s.RU);
    for (int u = tid; u < s.NU; u += BLOCK, k.step(s)) {
        const size_t e = chan + k.at<V>(s);
        Vec<V> r = ldv<V>(slab + (size_t)u * V);
        tn_unit<V>(a, e, r, mean, invstd, gamma, beta);
        stv<V>(a.y + e, r);
    }
}

// ---- forward, split regime, launch 1: grid (C, S); the slice stays in registers between its mean and its M2
template <int V>
__global__ __launch_bounds__(TN_BLOCK) void tn_stats_kernel(TnShape s, TnFwd a) {
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    constexpr int SU = TN_SLICE / V, PER = TN_PER / V;
    const int u0 = sl * SU, u1 = u0 + SU < s.NU ? u0 + SU : s.NU;
    if (sl >= s.S || u0 >= s.NU) return;
    const size_t chan = (size_t)c * s.HW;
    float r[TN_PER];
    float sum = 0.0f, m2 = 0.0f;
    TnWalk k(u0 + tid, s.RU);
#pragma unroll
    for (int p = 0; p < PER; ++p, k.step(s)) {
        const bool in = u0 + tid + p * TN_BLOCK < u1;
        Vec<V> q = {};
        if (in) q = ldv<V>(a.x + chan + k.at<V>(s));
#pragma unroll
        for (int j = 0; j < V; ++j) { r[p * V + j] = in ? q.v[j] : 0.0f; sum += r[p * V + j]; }
    }
    block_sum2<TN_BLOCK>(sum, m2, red);
    const float cnt = (float)((u1 - u0) * V);
    const float mean0 = sum / cnt;
    float rs = 0.0f;
    m2 = 0.0f;
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        const bool in = u0 + tid + p * TN_BLOCK < u1;
#pragma unroll
        for (int j = 0; j < V; ++j) { const float d = in ? r[p * V + j] - mean0 : 0.0f; rs += d; m2 += d * d; }
    }
    block_sum2<TN_BLOCK>(rs, m2, red);
    if (tid == 0) {
        const float dm = rs / cnt;
        a.ws[((size_t)c * s.S + sl) * 2] = mean0 + dm;
        a.ws[((size_t)c * s.S + sl) * 2 + 1] = fmaxf(m2 - rs * dm, 0.0f);
    }
}

// the S partials (mean, M2) of a channel merged by the first wave, in double: lane l takes the slices l, l + 64, ... in
// order, then the wave's butterfly; first the mean, then M2 around it (Chan's rule with the exact mean: M2 =
// sum M2_i + n_i (mean_i - mean)^2).  The same order, so the same value, in every workgroup of the channel.
__device__ inline void tn_merge_stats(const TnShape& s, const float* part, float eps, float& mean, float& var, float& invstd) {
    __shared__ double mrg[2];
    const int tid = threadIdx.x;
    if (tid < 64) {
        const double last = (double)(s.N - (s.S - 1) * TN_SLICE);
        double A = 0.0;
        for (int i = tid; i < s.S; i += 64) A += (i + 1 < s.S ? (double)TN_SLICE : last) * (double)part[2 * i];
        const double m = wave_sum_d(A) / (double)s.N;
        double Q = 0.0;
        for (int i = tid; i < s.S; i += 64) {
            const double d = (double)part[2 * i] - m;
            Q += (double)part[2 * i + 1] + (i + 1 < s.S ? (double)TN_SLICE : last) * d * d;
        }
        Q = wave_sum_d(Q);
        if (tid == 0) { mrg[0] = m; mrg[1] = Q; }
    }
    __syncthreads();
    const double mu = mrg[0], M2 = mrg[1];
    mean = (float)mu;
    var = (float)(M2 / (double)s.N);
    invstd = 1.0f / sqrtf(var + eps);
}

// mean and invstd of channel c in the apply kernels (grid (C, any)).  a.ws: the split regime's launch 2 merges the partials,
// and the workgroups with blockIdx.y == 0 publish; a.ws == NULL: the eval forward reads the running statistics
__device__ inline void tn_apply_stats(const TnShape& s, const TnFwd& a, int c, float& mean, float& invstd) {
    if (a.ws) {
        float var;
        tn_merge_stats(s, a.ws + (size_t)c * s.S * 2, a.eps, mean, var, invstd);
        if (blockIdx.y == 0 && threadIdx.x == 0) tn_publish(a, c, s.N, mean, var, invstd);
    } else {
        mean = a.rm[c];
        invstd = 1.0f / sqrtf(a.rv[c] + a.eps);
    }
}

// ---- forward, split regime launch 2 and the eval forward: grid (C, S), every workgroup normalises its slice
template <int V>
__global__ __launch_bounds__(TN_BLOCK) void tn_fwd_apply_kernel(TnShape s, TnFwd a) {
    const int c = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    constexpr int SU = TN_SLICE / V, PER = TN_PER / V;
    const int u0 = sl * SU, u1 = u0 + SU < s.NU ? u0 + SU : s.NU;
    if (sl >= s.S || u0 >= s.NU) return;
    float mean, invstd;
    tn_apply_stats(s, a, c, mean, invstd);
    const float gamma = a.w ? a.w[c] : 1.0f, beta = a.b ? a.b[c] : 0.0f;
    const size_t chan = (size_t)c * s.HW;
    TnWalk k(u0 + tid, s.RU);
    for (int p = 0; p < PER; ++p, k.step(s)) {
        if (u0 + tid + p * TN_BLOCK >= u1) break;
        const size_t e = chan + k.at<V>(s);
        Vec<V> r = ldv<V>(a.x + e);
        tn_unit<V>(a, e, r, mean, invstd, gamma, beta);
        stv<V>(a.y + e, r);
    }
}

// ---- backward.  A gradient source says what differs between the forms: load<V>() gives g, the upstream gradient of y
// before the norm, and xhat of the V elements of unit k of channel c, at element e; dres: the form has a d_residual (= g);
// onepass: the form has a one-pass regime.  It travels to the kernels by value next to TnShape / TnBwd.

// the ring: g = dy [y > 0] (the mask from the saved output, ATen's threshold backward)
struct ActGrad {
    static constexpr bool dres = true, onepass = true;
    template <int V>
    __device__ inline void load(const TnShape& s, const TnBwd& a, int c, const TnWalk& k, size_t e, float mean, float invstd,
                                Vec<V>& g, Vec<V>& xh) const {
        g = ldv<V>(a.dy + e);
        xh = ldv<V>(a.x + e);
        if (a.y) {
            const Vec<V> y = ldv<V>(a.y + e);
#pragma unroll
            for (int j = 0; j < V; ++j) g.v[j] = y.v[j] <= 0.0f ? 0.0f : g.v[j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) xh.v[j] = (xh.v[j] - mean) * invstd;
    }
};

__device__ inline void tn_bwd_stats(const TnBwd& a, int c, float& mean, float& invstd) {
    mean = a.stat_a[c];
    invstd = a.eval ? 1.0f / sqrtf(a.stat_b[c] + a.eps) : a.stat_b[c];
}

// ---- backward, one-pass regime: grid C; g and xhat of the channel stay in LDS between the two sums and dx
template <class SRC, int BLOCK, int V>
__global__ __launch_bounds__(BLOCK) void bwd_onepass_kernel(TnShape s, TnBwd a, SRC src) {
    constexpr int SLAB = BLOCK == 64 ? TN_SMALL : TN_MAX;
    __shared__ __attribute__((aligned(16))) float gs[SLAB];
    __shared__ __attribute__((aligned(16))) float xs[SLAB];
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (s.N > SLAB) return;
    float mean, invstd;
    tn_bwd_stats(a, c, mean, invstd);
    const size_t chan = (size_t)c * s.HW;
    float sg = 0.0f, sgx = 0.0f;
    {
        TnWalk k(tid, s.RU);
        for (int u = tid; u < s.NU; u += BLOCK, k.step(s)) {
            const size_t e = chan + k.at<V>(s);
            Vec<V> g, xh;
            src.template load<V>(s, a, c, k, e, mean, invstd, g, xh);
            stv<V>(gs + (size_t)u * V, g);
            stv<V>(xs + (size_t)u * V, xh);
            if constexpr (SRC::dres) { if (a.dres) stv<V>(a.dres + e, g); }
#pragma unroll
            for (int j = 0; j < V; ++j) { sg += g.v[j]; sgx += g.v[j] * xh.v[j]; }
        }
    }
    block_sum2<BLOCK>(sg, sgx, red);
    if (tid == 0) {
        if (a.db) a.db[c] = sg;
        if (a.dw) a.dw[c] = sgx;
    }
    if (!a.dx) return;
    const float kk = (a.w ? a.w[c] : 1.0f) * invstd;
    const float mg = a.eval ? 0.0f : sg / (float)s.N, mgx = a.eval ? 0.0f : sgx / (float)s.N;
    TnWalk k(tid, s.RU);
    for (int u = tid; u < s.NU; u += BLOCK, k.step(s)) {
        Vec<V> g = ldv<V>(gs + (size_t)u * V);
        const Vec<V> xh = ldv<V>(xs + (size_t)u * V);
#pragma unroll
        for (int j = 0; j < V; ++j) g.v[j] = kk * (g.v[j] - mg - xh.v[j] * mgx);
        stv<V>(a.dx + chan + k.at<V>(s), g);
    }
}

// ---- backward, split regime launch 1: grid (C, S); the two sums of a slice, and d_residual = g
template <class SRC, int V>
__global__ __launch_bounds__(TN_BLOCK) void bwd_partial_kernel(TnShape s, TnBwd a, SRC src) {
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    constexpr int SU = TN_SLICE / V, PER = TN_PER / V;
    const int u0 = sl * SU, u1 = u0 + SU < s.NU ? u0 + SU : s.NU;
    if (sl >= s.S || u0 >= s.NU) return;
    float mean, invstd;
    tn_bwd_stats(a, c, mean, invstd);
    const size_t chan = (size_t)c * s.HW;
    float sg = 0.0f, sgx = 0.0f;
    TnWalk k(u0 + tid, s.RU);
    for (int p = 0; p < PER; ++p, k.step(s)) {
        if (u0 + tid + p * TN_BLOCK >= u1) break;
        const size_t e = chan + k.at<V>(s);
        Vec<V> g, xh;
        src.template load<V>(s, a, c, k, e, mean, invstd, g, xh);
        if constexpr (SRC::dres) { if (a.dres) stv<V>(a.dres + e, g); }
#pragma unroll
        for (int j = 0; j < V; ++j) { sg += g.v[j]; sgx += g.v[j] * xh.v[j]; }
    }
    block_sum2<TN_BLOCK>(sg, sgx, red);
    if (tid == 0) {
        a.ws[((size_t)c * s.S + sl) * 2] = sg;
        a.ws[((size_t)c * s.S + sl) * 2 + 1] = sgx;
    }
}

// the S partials (sum g, sum g xhat) of a channel added by the first wave, in double: lane l takes the slices l, l + 64,
// ... in order, then the wave's butterfly: the same order, so the same value, in every workgroup of the channel
__device__ inline void tn_merge_sums(const TnShape& s, const float* part, float& sg, float& sgx) {
    __shared__ double mrg[2];
    const int tid = threadIdx.x;
    if (tid < 64) {
        double P = 0.0, Q = 0.0;
        for (int i = tid; i < s.S; i += 64) { P += (double)part[2 * i]; Q += (double)part[2 * i + 1]; }
        P = wave_sum_d(P); Q = wave_sum_d(Q);
        if (tid == 0) { mrg[0] = P; mrg[1] = Q; }
    }
    __syncthreads();
    const double A = mrg[0], Bx = mrg[1];
    sg = (float)A; sgx = (float)Bx;
}

// ---- backward, split regime launch 2, and the eval backward without affine gradients (a.sums == 0): grid (C, S), or
// (C, 1) when only the affine gradients are wanted (a.dx == NULL)
template <class SRC, int V>
__global__ __launch_bounds__(TN_BLOCK) void bwd_apply_kernel(TnShape s, TnBwd a, SRC src) {
    const int c = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    constexpr int SU = TN_SLICE / V, PER = TN_PER / V;
    const int u0 = sl * SU, u1 = u0 + SU < s.NU ? u0 + SU : s.NU;
    if (sl >= s.S || u0 >= s.NU) return;
    float sg = 0.0f, sgx = 0.0f;
    if (a.sums) {
        tn_merge_sums(s, a.ws + (size_t)c * s.S * 2, sg, sgx);
        if (sl == 0 && tid == 0) {
            if (a.db) a.db[c] = sg;
            if (a.dw) a.dw[c] = sgx;
        }
    }
    if (!a.dx) return;
    float mean, invstd;
    tn_bwd_stats(a, c, mean, invstd);
    const float kk = (a.w ? a.w[c] : 1.0f) * invstd;
    const float mg = a.eval ? 0.0f : sg / (float)s.N, mgx = a.eval ? 0.0f : sgx / (float)s.N;
    const size_t chan = (size_t)c * s.HW;
    TnWalk k(u0 + tid, s.RU);
    for (int p = 0; p < PER; ++p, k.step(s)) {
        if (u0 + tid + p * TN_BLOCK >= u1) break;
        const size_t e = chan + k.at<V>(s);
        Vec<V> g, xh;
        src.template load<V>(s, a, c, k, e, mean, invstd, g, xh);
#pragma unroll
        for (int j = 0; j < V; ++j) g.v[j] = kk * (g.v[j] - mg - xh.v[j] * mgx);
        stv<V>(a.dx + e, g);
    }
}

// ---- the stem's pool: max(tn_act(x), 0) and MaxPool2d(3, 2, 1) as one op.  Window (ph, pw) covers rows
// 2 ph - 1 .. 2 ph + 1 and columns 2 pw - 1 .. 2 pw + 1, taps outside the map take no part; p is the window's maximum and
// idx the tap number r * 3 + s of the first one.  Halo: none is staged; a work-item reads its window's taps from global
// memory and the overlap of neighbouring windows comes out of the cache (the windows of a workgroup are neighbours).
constexpr int TP_SLICE = VPN_BN_POOL_SLICE;     // pooled outputs of a channel a workgroup of tp_fwd_kernel owns
static_assert(TP_SLICE % (2 * TN_BLOCK) == 0, "a workgroup takes whole pairs of outputs per work-item");

// NP = B PH PW pooled outputs per channel, in SP slices of TP_SLICE
struct TpShape { int H, W, PH, PW, NP, SP; };

// the stem's activation: the ReLU is always on
__device__ inline float tp_act(float x, float mean, float invstd, float gamma, float beta) {
    return fmaxf(tn_act(x, mean, invstd, gamma, beta), 0.0f);
}

// ATen's rule: a tap replaces the best so far only if it is greater or is NaN, so the first maximum wins
__device__ inline void tp_tap(float& best, int& k, float y, int tap) {
    if (y > best || y != y) { best = y; k = tap; }
}

// window (ph, pw) of one map `m` (rows of W floats), taps scanned r then s ascending
__device__ inline void tp_window(const float* m, const TpShape& g, int ph, int pw, float mean, float invstd, float gamma,
                                 float beta, float& best, int& k) {
    best = -INFINITY; k = 0;
    for (int r = 0; r < 3; ++r) {
        const int h = 2 * ph - 1 + r;
        if (h < 0 || h >= g.H) continue;
        for (int t = 0; t < 3; ++t) {
            const int w = 2 * pw - 1 + t;
            if (w < 0 || w >= g.W) continue;
            tp_tap(best, k, tp_act(m[(size_t)h * g.W + w], mean, invstd, gamma, beta), r * 3 + t);
        }
    }
}

// ---- forward, one-pass regime: grid C; the statistics of tn_fwd_onepass_kernel, then the windows are read from the slab
// (element n of the channel = batch row n / HW, pixel n % HW)
template <int BLOCK, int V>
__global__ __launch_bounds__(BLOCK) void tp_fwd_onepass_kernel(TnShape s, TpShape g, TnFwd a, unsigned char* idx) {
    constexpr int SLAB = BLOCK == 64 ? TN_SMALL : TN_MAX;
    __shared__ __attribute__((aligned(16))) float slab[SLAB];
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (s.N > SLAB) return;
    float mean, var, invstd;
    tn_slab_stats<BLOCK, V>(s, a.x + (size_t)c * s.HW, a.eps, slab, red, mean, var, invstd);
    if (tid == 0) tn_publish(a, c, s.N, mean, var, invstd);
    __syncthreads();                                  // from here a work-item reads what others wrote to the slab
    const float gamma = a.w ? a.w[c] : 1.0f, beta = a.b ? a.b[c] : 0.0f;
    const int PHW = g.PH * g.PW;
    for (int o = tid; o < g.NP; o += BLOCK) {
        const int b = o / PHW, r = o - b * PHW, ph = r / g.PW, pw = r - ph * g.PW;
        float best; int k;
        tp_window(slab + (size_t)b * s.HW, g, ph, pw, mean, invstd, gamma, beta, best, k);
        const size_t e = ((size_t)b * s.C + c) * PHW + r;
        a.y[e] = best;
        idx[e] = (unsigned char)k;
    }
}

// ---- forward, split regime launch 2 (a.ws: merge the partials of tn_stats_kernel) and the eval forward (a.ws == NULL):
// grid (C, SP).  V = 4 (W a multiple of 4, x 16-byte aligned): a work-item takes the outputs (ph, pw), (ph, pw + 1) with pw
// even: of each row the four columns 2 pw .. 2 pw + 3 in one 16-byte access and column 2 pw - 1 by itself.
template <int V>
__global__ __launch_bounds__(TN_BLOCK) void tp_fwd_kernel(TnShape s, TpShape g, TnFwd a, unsigned char* idx) {
    const int c = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    constexpr int OUT = V == 4 ? 2 : 1;
    const int o0 = sl * TP_SLICE, o1 = o0 + TP_SLICE < g.NP ? o0 + TP_SLICE : g.NP;
    if (sl >= g.SP || o0 >= g.NP) return;
    float mean, invstd;
    tn_apply_stats(s, a, c, mean, invstd);
    const float gamma = a.w ? a.w[c] : 1.0f, beta = a.b ? a.b[c] : 0.0f;
    const int PHW = g.PH * g.PW;
    for (int o = o0 + tid * OUT; o < o1; o += TN_BLOCK * OUT) {
        const int b = o / PHW, r = o - b * PHW, ph = r / g.PW, pw = r - ph * g.PW;
        const float* m = a.x + ((size_t)b * s.C + c) * s.HW;
        const size_t e = ((size_t)b * s.C + c) * PHW + r;
        if (V == 4) {
            float b0 = -INFINITY, b1 = -INFINITY; int k0 = 0, k1 = 0;
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                const int h = 2 * ph - 1 + rr;
                if (h < 0 || h >= g.H) continue;
                const float* row = m + (size_t)h * g.W + 2 * pw;
                const Vec<4> q = ldv<4>(row);
                float y[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = tp_act(q.v[j], mean, invstd, gamma, beta);
                if (pw > 0) tp_tap(b0, k0, tp_act(row[-1], mean, invstd, gamma, beta), rr * 3);
                tp_tap(b0, k0, y[0], rr * 3 + 1); tp_tap(b0, k0, y[1], rr * 3 + 2);
                tp_tap(b1, k1, y[1], rr * 3); tp_tap(b1, k1, y[2], rr * 3 + 1); tp_tap(b1, k1, y[3], rr * 3 + 2);
            }
            a.y[e] = b0; a.y[e + 1] = b1;
            idx[e] = (unsigned char)k0; idx[e + 1] = (unsigned char)k1;
        } else {
            float best; int k;
            tp_window(m, g, ph, pw, mean, invstd, gamma, beta, best, k);
            a.y[e] = best;
            idx[e] = (unsigned char)k;
        }
    }
}

// upstream gradient of pixel (h, w) of the map whose pooled maps begin at element pc: dp [p > 0] of the at most four
// windows that hold the pixel and whose idx names it, ph then pw ascending.  a.dy: dp, a.y: p.
__device__ inline float tp_g(const TnBwd& a, const unsigned char* idx, const TpShape& g, size_t pc, int h, int w) {
    float sum = 0.0f;
    for (int ph = h >> 1; ph <= ((h + 1) >> 1) && ph < g.PH; ++ph) {
        const int r = h - 2 * ph + 1;
        for (int pw = w >> 1; pw <= ((w + 1) >> 1) && pw < g.PW; ++pw) {
            const size_t o = pc + (size_t)ph * g.PW + pw;
            const int k = idx[o];                         // the three loads do not wait for one another
            const float pv = a.y[o], dv = a.dy[o];
            sum += k == r * 3 + (w - 2 * pw + 1) && pv > 0.0f ? dv : 0.0f;
        }
    }
    return sum;
}

// the pool's gradient source: the input map is walked in slices at any N (no one-pass regime), a.dy is dp and a.y is p.
// V = 4: W is a multiple of 4, the four elements share a row
struct PoolGrad {
    static constexpr bool dres = false, onepass = false;
    TpShape g;
    const unsigned char* idx;
    template <int V>
    __device__ inline void load(const TnShape& s, const TnBwd& a, int c, const TnWalk& k, size_t e, float mean, float invstd,
                                Vec<V>& gr, Vec<V>& xh) const {
        const int i = k.i * V, h = i / g.W, w = i - h * g.W;
        const size_t pc = ((size_t)k.b * s.C + c) * g.PH * g.PW;
        xh = ldv<V>(a.x + e);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            gr.v[j] = tp_g(a, idx, g, pc, h, w + j);
            xh.v[j] = (xh.v[j] - mean) * invstd;
        }
    }
};

// ---- the trunk's tail: the last norm site also writes m[b,c] = (sum_hw y[b,c,hw]) / HW, the global
// average pool the heads read, and its backward takes m's gradient: upstream = dy + dm[b,c] / HW.  A row is the HW elements
// of one (batch row, channel).  Rows are summed from LDS where they fit: a group of G = 2^LG lanes (the smallest power of
// two >= min(HW, 64)) owns a row, lane j of the group adds the elements j, j + G, ... in order, then the group's butterfly.
// B: batch rows; RPB: rows a workgroup of tt_fwd_apply_kernel owns.
struct TtRows { int B, RPB, LG; };

// the means of `rows` rows of HW floats that lie one after another in LDS; row r goes to m[r * stride]
template <int BLOCK>
__device__ inline void tt_row_means(const float* slab, int rows, int HW, int LG, float* m, size_t stride) {
    const int lane = threadIdx.x & 63, G = 1 << LG, per = 64 >> LG, j = lane & (G - 1);
    for (int r0 = (threadIdx.x >> 6) * per; r0 < rows; r0 += (BLOCK / 64) * per) {      // the same trip count in a wave
        const int r = r0 + (lane >> LG);
        float v = 0.0f;
        if (r < rows) {
            const float* p = slab + (size_t)r * HW;
            for (int i = j; i < HW; i += G) v += p[i];
        }
        for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (r < rows && j == 0) m[(size_t)r * stride] = v / (float)HW;
    }
}

// ---- forward, one-pass regime: tn_fwd_onepass_kernel, with y written back to the slab and its rows summed from there
template <int BLOCK, int V>
__global__ __launch_bounds__(BLOCK) void tt_fwd_onepass_kernel(TnShape s, TtRows t, TnFwd a, float* m) {
    constexpr int SLAB = BLOCK == 64 ? TN_SMALL : TN_MAX;
    __shared__ __attribute__((aligned(16))) float slab[SLAB];
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (s.N > SLAB) return;
    const size_t chan = (size_t)c * s.HW;
    float mean, var, invstd;
    tn_slab_stats<BLOCK, V>(s, a.x + chan, a.eps, slab, red, mean, var, invstd);
    if (tid == 0) tn_publish(a, c, s.N, mean, var, invstd);
    const float gamma = a.w ? a.w[c] : 1.0f, beta = a.b ? a.b[c] : 0.0f;
    TnWalk k(tid, s.RU);
    for (int u = tid; u < s.NU; u += BLOCK, k.step(s)) {
        const size_t e = chan + k.at<V>(s);
        Vec<V> r = ldv<V>(slab + (size_t)u * V);
        tn_unit<V>(a, e, r, mean, invstd, gamma, beta);
        stv<V>(a.y + e, r);
        stv<V>(slab + (size_t)u * V, r);
    }
    __syncthreads();                                  // from here a work-item reads what others wrote to the slab
    tt_row_means<BLOCK>(slab, t.B, s.HW, t.LG, m + c, (size_t)s.C);
}

// ---- forward, split regime launch 2 and the eval forward: grid (C, ceil(B / RPB)), a workgroup owns the batch rows blockIdx.y * RPB ... of its channel.  HW <= TN_SLICE: RPB =
// TN_SLICE / HW rows, y staged in LDS and summed as above.  Longer rows: RPB = 1, a work-item adds its elements in unit
// order, then the workgroup's sum (block_sum2).
template <int V>
__global__ __launch_bounds__(TN_BLOCK) void tt_fwd_apply_kernel(TnShape s, TtRows t, TnFwd a, float* m) {
    __shared__ __attribute__((aligned(16))) float slab[TN_SLICE];
    __shared__ float red[2 * (TN_BLOCK / 64)];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int b0 = blockIdx.y * t.RPB, b1 = b0 + t.RPB < t.B ? b0 + t.RPB : t.B;
    if (b0 >= t.B) return;
    const bool staged = s.HW <= TN_SLICE;
    if (staged && (b1 - b0) * s.HW > TN_SLICE) return;          // the host never asks: nothing outside the slab either way
    float mean, invstd;
    tn_apply_stats(s, a, c, mean, invstd);
    const float gamma = a.w ? a.w[c] : 1.0f, beta = a.b ? a.b[c] : 0.0f;
    const size_t chan = (size_t)c * s.HW;
    const int u0 = b0 * s.RU, u1 = b1 * s.RU;
    float acc = 0.0f;
    TnWalk k(u0 + tid, s.RU);
    for (int u = u0 + tid; u < u1; u += TN_BLOCK, k.step(s)) {
        const size_t e = chan + k.at<V>(s);
        Vec<V> r = ldv<V>(a.x + e);
        tn_unit<V>(a, e, r, mean, invstd, gamma, beta);
        stv<V>(a.y + e, r);
        if (staged) {
            stv<V>(slab + (size_t)(u - u0) * V, r);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) acc += r.v[j];
        }
    }
    float* mr = m + (size_t)b0 * s.C + c;
    if (staged) {
        __syncthreads();
        tt_row_means<TN_BLOCK>(slab, b1 - b0, s.HW, t.LG, mr, (size_t)s.C);
    } else {
        float none = 0.0f;
        block_sum2<TN_BLOCK>(acc, none, red);
        if (tid == 0) mr[0] = acc / (float)s.HW;
    }
}

// the tail's gradient source: ActGrad on the upstream gradient dy + dm[b,c] / HW (a.dy or dm may be NULL: the other one
// alone)
struct TailGrad {
    static constexpr bool dres = true, onepass = true;
    const float* dm;
    template <int V>
    __device__ inline void load(const TnShape& s, const TnBwd& a, int c, const TnWalk& k, size_t e, float mean, float invstd,
                                Vec<V>& g, Vec<V>& xh) const {
        g = Vec<V>{};
        if (a.dy) g = ldv<V>(a.dy + e);
        if (dm) {
            const float q = dm[(size_t)k.b * s.C + c] / (float)s.HW;
#pragma unroll
            for (int j = 0; j < V; ++j) g.v[j] = a.dy ? g.v[j] + q : q;
        }
        xh = ldv<V>(a.x + e);
        if (a.y) {
            const Vec<V> y = ldv<V>(a.y + e);
#pragma unroll
            for (int j = 0; j < V; ++j) g.v[j] = y.v[j] <= 0.0f ? 0.0f : g.v[j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) xh.v[j] = (xh.v[j] - mean) * invstd;
    }
};

static bool tn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shape checks shared by the entry points; fills `s` for accesses of V floats and workgroups of `block` work-items
static int tn_shape(int B, int C, int H, int W, TnShape* s) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    const long long HW = (long long)H * W, N = HW * B;
    if (N > 2147483647LL || (N + TN_SLICE - 1) / TN_SLICE > 65535) return VPN_E_TOOBIG;
    s->C = C; s->HW = (int)HW; s->N = (int)N; s->S = (int)((N + TN_SLICE - 1) / TN_SLICE);
    return 0;
}

static void tn_units(TnShape* s, int V, int block) {
    s->RU = s->HW / V; s->NU = s->N / V;
    s->step_b = block / s->RU; s->step_i = block % s->RU;
}

// the split regime's [C, S, 2] partials, forward and backward
static size_t tn_workspace_bytes(const TnShape& s) { return (size_t)s.C * s.S * 2 * sizeof(float); }

static bool tn_workspace_ok(const TnShape& s, const void* workspace, size_t bytes) {
    return workspace && bytes >= tn_workspace_bytes(s) && !((uintptr_t)workspace & 3);
}

// the kernels' template ladders: f(V) with V = 4 (vec) or 1, and f(BLOCK, V) with BLOCK = 64 or TN_BLOCK, as integral
// constants, so that a launch is written once per kernel
template <int I> using TnInt = std::integral_constant<int, I>;
template <class F> static void tn_pick(bool vec, F f) {
    if (vec) f(TnInt<4>{});
    else f(TnInt<1>{});
}
template <class F> static void tn_pick(int block, bool vec, F f) {
    if (block == 64) tn_pick(vec, [&](auto V) { f(TnInt<64>{}, V); });
    else tn_pick(vec, [&](auto V) { f(TnInt<TN_BLOCK>{}, V); });
}

// what the three forwards check after their shape, and their TnFwd (`out`: y, or the pool's p).  a->ws says whether the
// regime is the split one.
static int tn_fwd_plan(const TnShape& s, const float* x, const float* residual, const float* weight, const float* bias,
                       float* running_mean, float* running_var, long long* num_batches_tracked, int training, float momentum,
                       float eps, int relu, float* out, float* save_mean, float* save_invstd, void* workspace,
                       size_t workspace_bytes, TnFwd* a) {
    if (!x || !out || !(eps >= 0.0f)) return VPN_E_BADARG;
    if (training ? (!save_mean || !save_invstd || s.N < 2 || !(momentum >= 0.0f && momentum <= 1.0f)) : (!running_mean || !running_var))
        return VPN_E_BADARG;
    const bool split = training && s.N > TN_MAX;
    if (split && !tn_workspace_ok(s, workspace, workspace_bytes)) return VPN_E_BADARG;
    *a = TnFwd{x, residual, weight, bias, running_mean, running_var, training ? num_batches_tracked : nullptr, out, save_mean,
               save_invstd, split ? (float*)workspace : nullptr, momentum, eps, relu != 0};
    return 0;
}

// the split regime's launch 1 of the three forwards; s in units of vec ? 4 : 1 and workgroups of TN_BLOCK
static int tn_launch_stats(const TnShape& s, const TnFwd& a, bool vec, hipStream_t st) {
    const dim3 grid((unsigned)s.C, (unsigned)s.S);
    tn_pick(vec, [&](auto V) { VPN_LAUNCH_AS("tn_stats_kernel", (tn_stats_kernel<V()>), grid, dim3(TN_BLOCK), 0, st, s, a); });
    VPN_LAUNCH_CHECK();
    return 0;
}

// vpn_bn_act_fwd (m == NULL) and vpn_bn_tail_fwd (m and its rows t) behind their shape checks
static int tn_ring_fwd(TnShape s, const TtRows* t, float* m, const float* x, const float* residual, const float* weight,
                       const float* bias, float* running_mean, float* running_var, long long* num_batches_tracked, int training,
                       float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, void* workspace,
                       size_t workspace_bytes, void* stream) {
    TnFwd a;
    const int rc = tn_fwd_plan(s, x, residual, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                               relu, y, save_mean, save_invstd, workspace, workspace_bytes, &a);
    if (rc) return rc;
    const bool vec = s.HW % 4 == 0 && tn_aligned16(x) && tn_aligned16(y) && tn_aligned16(residual);
    hipStream_t st = (hipStream_t)stream;
    if (training && !a.ws) {
        const int block = s.N <= TN_SMALL ? 64 : TN_BLOCK;
        tn_units(&s, vec ? 4 : 1, block);
        const dim3 grid((unsigned)s.C);
        tn_pick(block, vec, [&](auto BLOCK, auto V) {
            if (m) VPN_LAUNCH_AS("tt_fwd_onepass_kernel", (tt_fwd_onepass_kernel<BLOCK(), V()>), grid, dim3(BLOCK()), 0, st, s, *t, a, m);
            else VPN_LAUNCH_AS("tn_fwd_onepass_kernel", (tn_fwd_onepass_kernel<BLOCK(), V()>), grid, dim3(BLOCK()), 0, st, s, a);
        });
        VPN_LAUNCH_CHECK();
        return 0;
    }
    tn_units(&s, vec ? 4 : 1, TN_BLOCK);
    if (a.ws) {
        const int rs = tn_launch_stats(s, a, vec, st);
        if (rs) return rs;
    }
    tn_pick(vec, [&](auto V) {
        if (m) {
            const dim3 grid((unsigned)s.C, (unsigned)((t->B + t->RPB - 1) / t->RPB));
            VPN_LAUNCH_AS("tt_fwd_apply_kernel", (tt_fwd_apply_kernel<V()>), grid, dim3(TN_BLOCK), 0, st, s, *t, a, m);
        } else {
            const dim3 grid((unsigned)s.C, (unsigned)s.S);
            VPN_LAUNCH_AS("tn_fwd_apply_kernel", (tn_fwd_apply_kernel<V()>), grid, dim3(TN_BLOCK), 0, st, s, a);
        }
    });
    VPN_LAUNCH_CHECK();
    return 0;
}

struct TnLabels { const char *onepass, *partial, *apply; };        // the launch labels of a form's backward

// the backward of all three forms behind the form's own pointer checks.  `a` comes with its pointers and eps; ws, eval and
// sums are set here.  A form without a one-pass regime is in the split regime at any N.
template <class SRC>
static int tn_bwd(const TnLabels& L, const SRC& src, TnShape s, TnBwd a, int training, bool vec, void* workspace,
                  size_t workspace_bytes, void* stream) {
    if (!a.x || !a.stat_a || !a.stat_b || !(a.eps >= 0.0f) || (training && s.N < 2)) return VPN_E_BADARG;
    const bool affine = a.dw || a.db;
    if (!a.dx && !a.dres && !affine) return 0;                       // nothing is wanted
    const bool sums = training || affine;                            // eval: dx needs no sum
    const bool split = !SRC::onepass || s.N > TN_MAX;
    const bool partial = sums || a.dres;                             // split regime: launch 1 forms the sums and writes d_residual
    if (split && partial && !tn_workspace_ok(s, workspace, workspace_bytes)) return VPN_E_BADARG;
    a.ws = split && partial ? (float*)workspace : nullptr;
    a.eval = training ? 0 : 1;
    a.sums = split && sums ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if constexpr (SRC::onepass) {
        if (!split) {
            const int block = s.N <= TN_SMALL ? 64 : TN_BLOCK;
            tn_units(&s, vec ? 4 : 1, block);
            const dim3 grid((unsigned)s.C);
            tn_pick(block, vec, [&](auto BLOCK, auto V) {
                VPN_LAUNCH_AS(L.onepass, (bwd_onepass_kernel<SRC, BLOCK(), V()>), grid, dim3(BLOCK()), 0, st, s, a, src);
            });
            VPN_LAUNCH_CHECK();
            return 0;
        }
    }
    tn_units(&s, vec ? 4 : 1, TN_BLOCK);
    const dim3 grid((unsigned)s.C, (unsigned)s.S);
    if (partial) {
        tn_pick(vec, [&](auto V) { VPN_LAUNCH_AS(L.partial, (bwd_partial_kernel<SRC, V()>), grid, dim3(TN_BLOCK), 0, st, s, a, src); });
        VPN_LAUNCH_CHECK();
    }
    if (a.dx || affine) {
        const dim3 g2 = a.dx ? grid : dim3((unsigned)s.C, 1u);
        tn_pick(vec, [&](auto V) { VPN_LAUNCH_AS(L.apply, (bwd_apply_kernel<SRC, V()>), g2, dim3(TN_BLOCK), 0, st, s, a, src); });
        VPN_LAUNCH_CHECK();
    }
    return 0;
}

// vpn_bn_act_bwd and vpn_bn_tail_bwd behind their shape checks and the check of their upstream gradients
template <class SRC>
static int tn_ring_bwd(const TnLabels& L, const SRC& src, const TnShape& s, const float* dy, const float* x, const float* y,
                       const float* weight, const float* stat_mean, const float* stat_var, int training, float eps, int relu,
                       float* dx, float* d_residual, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (relu && !y) return VPN_E_BADARG;
    const TnBwd a{dy, x, relu ? y : nullptr, weight, stat_mean, stat_var, dx, d_residual, d_weight, d_bias, nullptr, eps, 0, 0};
    const bool vec = s.HW % 4 == 0 && tn_aligned16(dy) && tn_aligned16(x) && tn_aligned16(a.y) && tn_aligned16(dx) &&
                     tn_aligned16(d_residual);
    return tn_bwd(L, src, s, a, training, vec, workspace, workspace_bytes, stream);
}

// shape checks of the pool's entry points on top of tn_shape
static int tp_shape(int B, int C, int H, int W, TnShape* s, TpShape* g) {
    const int rc = tn_shape(B, C, H, W, s);
    if (rc) return rc;
    g->H = H; g->W = W; g->PH = (H - 1) / 2 + 1; g->PW = (W - 1) / 2 + 1;
    const long long NP = (long long)B * g->PH * g->PW, SP = (NP + TP_SLICE - 1) / TP_SLICE;
    if (SP > 65535) return VPN_E_TOOBIG;
    g->NP = (int)NP; g->SP = (int)SP;
    return 0;
}

// the rows of the tail's entry points on top of tn_shape: whole batch rows per workgroup of tt_fwd_apply_kernel
static int tt_shape(int B, int C, int H, int W, TnShape* s, TtRows* t) {
    const int rc = tn_shape(B, C, H, W, s);
    if (rc) return rc;
    t->B = B;
    t->RPB = s->HW <= TN_SLICE ? TN_SLICE / s->HW : 1;
    if ((B + t->RPB - 1) / t->RPB > 65535) return VPN_E_TOOBIG;
    t->LG = 0;
    while (t->LG < 6 && (1 << t->LG) < s->HW) ++t->LG;
    return 0;
}

}  // namespace vpn

using namespace vpn;

extern "C" size_t vpn_bn_act_workspace(int B, int C, int H, int W) {
    TnShape s;
    if (tn_shape(B, C, H, W, &s) != 0 || s.N <= TN_MAX) return 0;
    return tn_workspace_bytes(s);
}

extern "C" int vpn_bn_act_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* running_mean,
                              float* running_var, long long* num_batches_tracked, int B, int C, int H, int W, int training,
                              float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, void* workspace,
                              size_t workspace_bytes, void* stream) {
    TnShape s;
    const int rc = tn_shape(B, C, H, W, &s);
    if (rc) return rc;
    return tn_ring_fwd(s, nullptr, nullptr, x, residual, weight, bias, running_mean, running_var, num_batches_tracked, training,
                       momentum, eps, relu, y, save_mean, save_invstd, workspace, workspace_bytes, stream);
}

extern "C" int vpn_bn_act_bwd(const float* dy, const float* x, const float* y, const float* weight, const float* stat_mean,
                              const float* stat_var, int B, int C, int H, int W, int training, float eps, int relu, float* dx,
                              float* d_residual, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                              void* stream) {
    static const TnLabels L{"tn_bwd_onepass_kernel", "tn_bwd_partial_kernel", "tn_bwd_apply_kernel"};
    TnShape s;
    const int rc = tn_shape(B, C, H, W, &s);
    if (rc) return rc;
    if (!dy) return VPN_E_BADARG;
    return tn_ring_bwd(L, ActGrad{}, s, dy, x, y, weight, stat_mean, stat_var, training, eps, relu, dx, d_residual, d_weight, d_bias,
                       workspace, workspace_bytes, stream);
}

extern "C" size_t vpn_bn_pool_workspace(int B, int C, int H, int W) {
    TnShape s;
    TpShape g;
    if (tp_shape(B, C, H, W, &s, &g) != 0) return 0;
    return tn_workspace_bytes(s);
}

extern "C" int vpn_bn_pool_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                               long long* num_batches_tracked, int B, int C, int H, int W, int training, float momentum, float eps,
                               float* p, unsigned char* idx, float* save_mean, float* save_invstd, void* workspace,
                               size_t workspace_bytes, void* stream) {
    TnShape s;
    TpShape g;
    int rc = tp_shape(B, C, H, W, &s, &g);
    if (rc) return rc;
    if (!idx) return VPN_E_BADARG;
    TnFwd a;
    rc = tn_fwd_plan(s, x, nullptr, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps, 1, p,
                     save_mean, save_invstd, workspace, workspace_bytes, &a);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = s.HW % 4 == 0 && tn_aligned16(x);              // how the statistics read x; the pool asks for W % 4 == 0
    const int block = training && s.N <= TN_SMALL ? 64 : TN_BLOCK;
    tn_units(&s, vec ? 4 : 1, block);
    if (training && !a.ws) {
        const dim3 grid((unsigned)C);
        tn_pick(block, vec, [&](auto BLOCK, auto V) {
            VPN_LAUNCH_AS("tp_fwd_onepass_kernel", (tp_fwd_onepass_kernel<BLOCK(), V()>), grid, dim3(BLOCK()), 0, st, s, g, a, idx);
        });
        VPN_LAUNCH_CHECK();
        return 0;
    }
    if (a.ws) {
        rc = tn_launch_stats(s, a, vec, st);
        if (rc) return rc;
    }
    const dim3 grid((unsigned)C, (unsigned)g.SP);
    tn_pick(vec && W % 4 == 0, [&](auto V) {
        VPN_LAUNCH_AS("tp_fwd_kernel", (tp_fwd_kernel<V()>), grid, dim3(TN_BLOCK), 0, st, s, g, a, idx);
    });
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_bn_pool_bwd(const float* dp, const float* x, const float* p, const unsigned char* idx, const float* weight,
                               const float* stat_mean, const float* stat_var, int B, int C, int H, int W, int training, float eps,
                               float* dx, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes, void* stream) {
    static const TnLabels L{nullptr, "tp_bwd_partial_kernel", "tp_bwd_apply_kernel"};
    TnShape s;
    TpShape g;
    const int rc = tp_shape(B, C, H, W, &s, &g);
    if (rc) return rc;
    if (!dp || !p || !idx) return VPN_E_BADARG;
    const TnBwd a{dp, x, p, weight, stat_mean, stat_var, dx, nullptr, d_weight, d_bias, nullptr, eps, 0, 0};
    const bool vec = W % 4 == 0 && tn_aligned16(x) && tn_aligned16(dx);
    return tn_bwd(L, PoolGrad{g, idx}, s, a, training, vec, workspace, workspace_bytes, stream);
}

extern "C" size_t vpn_bn_tail_workspace(int B, int C, int H, int W) {
    TnShape s;
    TtRows t;
    if (tt_shape(B, C, H, W, &s, &t) != 0 || s.N <= TN_MAX) return 0;
    return tn_workspace_bytes(s);
}

extern "C" int vpn_bn_tail_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* running_mean,
                               float* running_var, long long* num_batches_tracked, int B, int C, int H, int W, int training,
                               float momentum, float eps, int relu, float* y, float* m, float* save_mean, float* save_invstd,
                               void* workspace, size_t workspace_bytes, void* stream) {
    TnShape s;
    TtRows t;
    const int rc = tt_shape(B, C, H, W, &s, &t);
    if (rc) return rc;
    if (!m) return VPN_E_BADARG;
    return tn_ring_fwd(s, &t, m, x, residual, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                       relu, y, save_mean, save_invstd, workspace, workspace_bytes, stream);
}

extern "C" int vpn_bn_tail_bwd(const float* dy, const float* dm, const float* x, const float* y, const float* weight,
                               const float* stat_mean, const float* stat_var, int B, int C, int H, int W, int training, float eps,
                               int relu, float* dx, float* d_residual, float* d_weight, float* d_bias, void* workspace,
                               size_t workspace_bytes, void* stream) {
    static const TnLabels L{"tt_bwd_onepass_kernel", "tt_bwd_partial_kernel", "tt_bwd_apply_kernel"};
    TnShape s;
    TtRows t;
    const int rc = tt_shape(B, C, H, W, &s, &t);
    if (rc) return rc;
    if (!dy && !dm) return VPN_E_BADARG;
    return tn_ring_bwd(L, TailGrad{dm}, s, dy, x, y, weight, stat_mean, stat_var, training, eps, relu, dx, d_residual, d_weight,
                       d_bias, workspace, workspace_bytes, stream);
}
