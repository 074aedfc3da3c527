// occloss.hip — the occupancy loss of a primitive assembly: the soft union of K primitives against occupancy
// labels at query points, with an overlap penalty, both ways.  The definition is in include/vpn_hip.h (vpn_occloss_fwd).
//
//   occl_fwd_kernel         prim_field_kernel's grid and staging: one work-item per (query, sample), the records of 256
//                           primitives at a time in LDS, read as broadcasts.  An online log-sum-exp over z_k = -(m_k - 1) / tau
//                           and the overlap sum of sigmoid(z_k); lse [B,Q] and s [B,Q]; one row (sum bce, sum ov, skipped) per
//                           workgroup: xor tree over the wave, the four waves (0 + 1) + (2 + 3).
//   occl_fwd_finish_kernel  ONE workgroup: lane t adds rows t, t + 256, ... in fp64, the 256 lanes by a tree in LDS; out [2] and
//                           n_skipped.
//   occl_bwd_kernel         one workgroup per (query slice, sample), a slice = 256 qpl queries (vpn_occloss_plan).  A lane keeps
//                           its qpl <= 8 queries in registers (x and the two per-query factors of c_k), loops over the staged
//                           primitives, accumulates the twelve sums (sum gamma, sum gamma (x) x~) of a primitive over its own
//                           queries and reduces them once per primitive over its wave; lane 0 of EVERY WAVE writes a row of
//                           partial [B][slices][4][K][12]: no barrier but the staging's, no hand-off between waves.
//   occl_bwd_finish_kernel  per (b, k): sixteen lanes, twelve of which add the 4 slices rows in ascending order in fp64; the
//                           chain rule to (v, q, t) through pose_backward; dparams [B,K,10].
//
// No atomics, no scratch, nothing allocated, no host synchronisation: capturable and bit-equal from run to run.
//
// Built with -ffp-contract=off: m_k is formed exactly as prim_field_kernel forms it (occupancy_prim.h), so for K = 1 the logit is
// -(field) / tau bit for bit.
#include "vpn_common.h"
#include "occupancy_prim.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int OL_TILE = VPN_OCCUPANCY_TILE;             // queries per workgroup of the forward; lanes of a backward workgroup
constexpr int OL_MAX_ITEMS = VPN_OCCUPANCY_MAX_ITEMS;
constexpr int OL_MAX_QPL = VPN_OCCLOSS_MAX_QPL;         // queries a lane of the backward keeps in registers, at most
constexpr int OL_MIN_GROUPS = VPN_OCCLOSS_MIN_GROUPS;   // the backward halves the slice until it has this many workgroups
constexpr int OL_SUMS = 12;
using vpn::OC_STAGE;
using vpn::OcPrim;

__device__ inline bool ol_finite(float v) { return fabsf(v) <= FLT_MAX; }    // false for a NaN

// m_k of a point in local coordinates: prim_field_kernel's expression
__device__ inline float ol_measure(const OcPrim& p, const vpn::F3& y) {
    return p.sphere ? y.x * y.x + y.y * y.y + y.z * y.z
                    : ((y.x != y.x || y.y != y.y || y.z != y.z) ? NAN : fmaxf(fabsf(y.x), fmaxf(fabsf(y.y), fabsf(y.z))));
}

// 1 / (1 + exp(-z)) for z >= 0, exp(z) / (1 + exp(z)) below
__device__ inline float ol_sigmoid(float z) {
    const float e = expf(-fabsf(z));
    return (z >= 0.0f ? 1.0f : e) / (1.0f + e);
}

__device__ inline float ol_label(const void* __restrict__ labels, int labels_u8, size_t at) {
    return labels_u8 ? (static_cast<const uint8_t*>(labels)[at] ? 1.0f : 0.0f) : static_cast<const float*>(labels)[at];
}

// queries [Q,3] (q_stride 0) or [B,Q,3] (q_stride 3 Q); labels [B,Q] or NULL (then rows is not written either); lse, s [B,Q] or
// NULL; rows [B][blocks][4], blocks the grid's x
__global__ __launch_bounds__(256) void occl_fwd_kernel(const float* __restrict__ params, const int32_t* __restrict__ kinds,
                                                       const float* __restrict__ queries, long long q_stride,
                                                       const void* __restrict__ labels, int labels_u8, int K, int Q, int blocks,
                                                       float tau, float* __restrict__ lse, float* __restrict__ s,
                                                       float* __restrict__ rows) {
    __shared__ OcPrim s_p[OC_STAGE];
    __shared__ float s_w[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, i = blockIdx.x * OL_TILE + tid;
    const bool valid = i < Q;
    const vpn::F3 x = valid ? vpn::ld3(queries + (size_t)b * q_stride + (size_t)i * 3) : vpn::F3{0.0f, 0.0f, 0.0f};
    float zmax = -INFINITY, sum = 0.0f, overlap = 0.0f;
    for (int base = 0; base < K; base += OC_STAGE) {
        const int m = min(OC_STAGE, K - base);
        __syncthreads();                                 // the previous records have been read
        if (tid < m) vpn::oc_stage_prim(s_p[tid], params, kinds, b, K, base + tid);
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const OcPrim& p = s_p[k];                    // the same address for every lane: an LDS broadcast
            const float mk = ol_measure(p, vpn::oc_local(p, x));
            if (!ol_finite(mk)) continue;
            const float d = mk - 1.0f;
            const float z = -d / tau;
            if (!(z > -INFINITY)) continue;              // exp(-inf) and sigmoid(-inf) are 0: nothing to add
            if (z > zmax) { sum = sum * expf(zmax - z) + 1.0f; zmax = z; }
            else sum += expf(z - zmax);
            overlap += ol_sigmoid(z);
        }
    }
    const float l = zmax == INFINITY ? INFINITY : (sum > 0.0f ? zmax + logf(sum) : -INFINITY);
    if (valid && lse) { lse[(size_t)b * Q + i] = l; s[(size_t)b * Q + i] = overlap; }
    if (!labels) return;                                 // uniform: the soft occupancy alone
    float bce = 0.0f, ov = 0.0f, skipped = 0.0f;
    if (valid) {
        const float y = ol_label(labels, labels_u8, (size_t)b * Q + i);
        if (ol_finite(x.x) && ol_finite(x.y) && ol_finite(x.z) && y == y && ol_finite(l)) {
            bce = (fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l)))) - y * l;
            const float r = overlap - 1.0f;
            ov = r > 0.0f ? r * r : 0.0f;
        } else {
            skipped = 1.0f;
        }
    }
    bce = vpn::wave_sum(bce); ov = vpn::wave_sum(ov); skipped = vpn::wave_sum(skipped);
    if (lane == 0) { s_w[wave][0] = bce; s_w[wave][1] = ov; s_w[wave][2] = skipped; }
    __syncthreads();
    if (tid < 4) rows[((size_t)b * blocks + blockIdx.x) * 4 + tid] = tid < 3 ? (s_w[0][tid] + s_w[1][tid]) + (s_w[2][tid] + s_w[3][tid]) : 0.0f;
}

// ONE workgroup.  out [2] = (sum bce, sum ov) / count; n_skipped [1] or NULL
__global__ __launch_bounds__(256) void occl_fwd_finish_kernel(const float* __restrict__ rows, long long n_rows, double count,
                                                              float* __restrict__ out, int32_t* __restrict__ n_skipped) {
    __shared__ double s_d[3][256];
    const int tid = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (long long r = tid; r < n_rows; r += 256) {
        a0 += (double)rows[(size_t)r * 4]; a1 += (double)rows[(size_t)r * 4 + 1]; a2 += (double)rows[(size_t)r * 4 + 2];
    }
    s_d[0][tid] = a0; s_d[1][tid] = a1; s_d[2][tid] = a2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s_d[0][tid] += s_d[0][tid + o]; s_d[1][tid] += s_d[1][tid + o]; s_d[2][tid] += s_d[2][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = (float)(s_d[0][0] / count);
        out[1] = (float)(s_d[1][0] / count);
        if (n_skipped) n_skipped[0] = s_d[2][0] >= (double)INT_MAX ? INT_MAX : (int32_t)s_d[2][0];
    }
}

struct OlPlan { int qpl, slice, slices; };

// a function of (B, Q) alone: the largest qpl in 8, 4, 2, 1 that still gives OL_MIN_GROUPS workgroups, else 1
inline OlPlan occl_plan(int B, int Q) {
    OlPlan pl;
    pl.qpl = OL_MAX_QPL;
    while (pl.qpl > 1 && (long long)B * ((Q + OL_TILE * pl.qpl - 1) / (OL_TILE * pl.qpl)) < OL_MIN_GROUPS) pl.qpl >>= 1;
    pl.slice = OL_TILE * pl.qpl;
    pl.slices = (Q + pl.slice - 1) / pl.slice;
    return pl;
}

// partial [B][slices][4][K][12]: per wave, per primitive (sum gamma [3], sum gamma_i x~_l [3][3]), gamma = dL/dx~
__global__ __launch_bounds__(256) void occl_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ params,
                                                       const int32_t* __restrict__ kinds, const float* __restrict__ queries,
                                                       long long q_stride, const void* __restrict__ labels, int labels_u8,
                                                       const float* __restrict__ lse, const float* __restrict__ s, int K, int Q,
                                                       int qpl, int slices, float tau, double count, float* __restrict__ partial) {
    __shared__ OcPrim s_p[OC_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const float g0 = grad[0], g1 = grad[1];
    vpn::F3 xq[OL_MAX_QPL];
    float lq[OL_MAX_QPL], aq[OL_MAX_QPL], bq[OL_MAX_QPL];
#pragma unroll
    for (int j = 0; j < OL_MAX_QPL; ++j) {
        xq[j] = vpn::F3{NAN, NAN, NAN}; lq[j] = 0.0f; aq[j] = 0.0f; bq[j] = 0.0f;      // a NaN query meets no primitive
        const long long i = ((long long)blockIdx.x * qpl + j) * OL_TILE + tid;
        if (j < qpl && i < Q) {
            const size_t at = (size_t)b * Q + (size_t)i;
            const vpn::F3 x = vpn::ld3(queries + (size_t)b * q_stride + (size_t)i * 3);
            const float y = ol_label(labels, labels_u8, at), l = lse[at];
            if (ol_finite(x.x) && ol_finite(x.y) && ol_finite(x.z) && y == y && ol_finite(l)) {
                const float r = s[at] - 1.0f;
                xq[j] = x; lq[j] = l;
                // dL/dm_k = -c_k / tau: the two factors of c_k that belong to the query, over B Q (the exact count, in fp64, as
                // the forward divides) and over -tau
                aq[j] = -((float)((double)(g0 * (ol_sigmoid(l) - y)) / count) / tau);
                bq[j] = -((float)((double)(g1 * (2.0f * (r > 0.0f ? r : 0.0f))) / count) / tau);
            }
        }
    }
    float* row0 = partial + (((size_t)b * slices + blockIdx.x) * 4 + wave) * (size_t)K * OL_SUMS;
    for (int base = 0; base < K; base += OC_STAGE) {
        const int m = min(OC_STAGE, K - base);
        __syncthreads();
        if (tid < m) vpn::oc_stage_prim(s_p[tid], params, kinds, b, K, base + tid);
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const OcPrim& p = s_p[k];
            float acc[OL_SUMS];
#pragma unroll
            for (int c = 0; c < OL_SUMS; ++c) acc[c] = 0.0f;
#pragma unroll
            for (int j = 0; j < OL_MAX_QPL; ++j) {
                if (j < qpl) {                           // uniform
                    const vpn::F3 y = vpn::oc_local(p, xq[j]);
                    const float mk = ol_measure(p, y);
                    if (ol_finite(mk)) {
                        const float d = mk - 1.0f;
                        const float z = -d / tau;
                        const float sg = ol_sigmoid(z);
                        const float dm = aq[j] * expf(z - lq[j]) + bq[j] * (sg * (1.0f - sg));
                        float gx, gy, gz;
                        if (p.sphere) {
                            gx = dm * (2.0f * y.x); gy = dm * (2.0f * y.y); gz = dm * (2.0f * y.z);
                        } else {                         // the lowest axis that attains the maximum; sign(0) = 0
                            const float ax = fabsf(y.x), ay = fabsf(y.y), az = fabsf(y.z);
                            const int a = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
                            const float v = a == 0 ? y.x : (a == 1 ? y.y : y.z);
                            const float sgn = v > 0.0f ? dm : (v < 0.0f ? -dm : 0.0f);
                            gx = a == 0 ? sgn : 0.0f; gy = a == 1 ? sgn : 0.0f; gz = a == 2 ? sgn : 0.0f;
                        }
                        acc[0] += gx; acc[1] += gy; acc[2] += gz;
                        acc[3] += gx * y.x; acc[4] += gx * y.y; acc[5] += gx * y.z;
                        acc[6] += gy * y.x; acc[7] += gy * y.y; acc[8] += gy * y.z;
                        acc[9] += gz * y.x; acc[10] += gz * y.y; acc[11] += gz * y.z;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < OL_SUMS; ++c) acc[c] = vpn::wave_sum(acc[c]);
            if (lane == 0) {
                float* row = row0 + (size_t)(base + k) * OL_SUMS;
#pragma unroll
                for (int c = 0; c < OL_SUMS; ++c) row[c] = acc[c];
            }
        }
    }
}

// 64 lanes = four (b, k) of sixteen lanes; n_rows = 4 slices rows a (b, k)
__global__ __launch_bounds__(64) void occl_bwd_finish_kernel(const float* __restrict__ partial, const float* __restrict__ params,
                                                             int BK, int K, int n_rows, float* __restrict__ dparams) {
    __shared__ double s_s[4][OL_SUMS];
    const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15;
    const long long bk = (long long)blockIdx.x * 4 + grp;
    if (bk < BK && c < OL_SUMS) {
        const int b = (int)(bk / K), k = (int)(bk - (long long)b * K);
        const float* src = partial + ((size_t)b * n_rows * K + k) * OL_SUMS + c;
        double acc = 0.0;
        for (int r = 0; r < n_rows; ++r) acc += (double)src[(size_t)r * K * OL_SUMS];
        s_s[grp][c] = acc;
    }
    __syncthreads();
    if (bk < BK && c == 0) {
        const float* prm = params + (size_t)bk * VPN_PARAM_STRIDE;
        float* out = dparams + (size_t)bk * VPN_PARAM_STRIDE;
        const vpn::Pose pose = vpn::make_pose(prm[3], prm[4], prm[5], prm[6]);
        const double* S = s_s[grp];
        bool live = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            live = live && ol_finite(prm[i]) && prm[i] != 0.0f && ol_finite(prm[7 + i]);
#pragma unroll
            for (int j = 0; j < 3; ++j) live = live && ol_finite(pose.R.m[i][j]);
        }
        if (!live) {                                     // every m_k of such a primitive was skipped: its sums are 0
#pragma unroll
            for (int i = 0; i < VPN_PARAM_STRIDE; ++i) out[i] = 0.0f;
            return;
        }
        const double v[3] = {(double)prm[0], (double)prm[1], (double)prm[2]};
        float g[3][3], gq[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // dL/dt_j = -sum_i R[j][i] (sum gamma_i) / v_i
            out[7 + j] = (float)(-(((double)pose.R.m[j][0] * (S[0] / v[0]) + (double)pose.R.m[j][1] * (S[1] / v[1])) +
                                   (double)pose.R.m[j][2] * (S[2] / v[2])));
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                // dL/dR[j][i] = sum_l R[j][l] v_l G[i][l] / v_i
                const double* G = S + 3 + 3 * i;
                g[j][i] = (float)(((((double)pose.R.m[j][0] * v[0]) * G[0] + ((double)pose.R.m[j][1] * v[1]) * G[1]) +
                                   ((double)pose.R.m[j][2] * v[2]) * G[2]) / v[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = (float)(-(S[3 + 4 * i] / v[i]));      // dL/dv_i = -G[i][i] / v_i
        vpn::pose_backward(pose, prm[3], prm[4], prm[5], g, gq);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[3 + i] = gq[i];
    }
}

int occl_check(int B, int K, int Q) {
    if (B <= 0 || K <= 0 || Q <= 0) return VPN_E_BADARG;
    if (B > 65535 || Q > OL_MAX_ITEMS || K > VPN_MAX_PRIMS) return VPN_E_TOOBIG;
    return 0;
}

inline size_t occl_fwd_bytes(int B, int Q) { return (size_t)B * ((Q + OL_TILE - 1) / OL_TILE) * 4 * sizeof(float); }
inline size_t occl_bwd_bytes(int B, int K, int Q) { return (size_t)B * occl_plan(B, Q).slices * 4 * K * OL_SUMS * sizeof(float); }

}  // namespace

extern "C" int vpn_occloss_plan(int B, int Q, int* slice_queries) {
    const int rc = occl_check(B, 1, Q);
    if (rc) return rc;
    const OlPlan pl = occl_plan(B, Q);
    if (slice_queries) *slice_queries = pl.slice;
    return pl.slices;
}

extern "C" size_t vpn_occloss_workspace(int B, int K, int Q) {
    if (occl_check(B, K, Q)) return 0;
    const size_t f = occl_fwd_bytes(B, Q), w = occl_bwd_bytes(B, K, Q);
    return ((f > w ? f : w) + 15) & ~(size_t)15;
}

extern "C" int vpn_occloss_fwd(const float* params, const int32_t* kinds, const float* queries, int shared_queries,
                               const void* labels, int labels_u8, int B, int K, int Q, float tau, void* workspace,
                               size_t workspace_bytes, float* lse, float* s, float* out, int32_t* n_skipped, void* stream) {
    if (!params || !kinds || !queries) return VPN_E_BADARG;
    if ((lse == nullptr) != (s == nullptr) || (!lse && !out)) return VPN_E_BADARG;
    if (out ? (!labels || !workspace) : n_skipped != nullptr) return VPN_E_BADARG;
    if (!(tau > 0.0f && tau <= FLT_MAX)) return VPN_E_BADARG;
    const int rc = occl_check(B, K, Q);
    if (rc) return rc;
    if (out && (workspace_bytes < occl_fwd_bytes(B, Q) || (reinterpret_cast<uintptr_t>(workspace) & 15))) return VPN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (Q + OL_TILE - 1) / OL_TILE;
    float* rows = static_cast<float*>(workspace);
    VPN_LAUNCH(occl_fwd_kernel, dim3(blocks, B), dim3(256), 0, st, params, kinds, queries, shared_queries ? 0LL : 3LL * Q,
               out ? labels : (const void*)nullptr, labels_u8, K, Q, blocks, tau, lse, s, rows);
    if (out)
        VPN_LAUNCH(occl_fwd_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)rows, (long long)B * blocks,
                   (double)B * (double)Q, out, n_skipped);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_occloss_bwd(const float* grad, const float* params, const int32_t* kinds, const float* queries,
                               int shared_queries, const void* labels, int labels_u8, const float* lse, const float* s, int B,
                               int K, int Q, float tau, void* workspace, size_t workspace_bytes, float* dparams, void* stream) {
    if (!grad || !params || !kinds || !queries || !labels || !lse || !s || !workspace || !dparams) return VPN_E_BADARG;
    if (!(tau > 0.0f && tau <= FLT_MAX)) return VPN_E_BADARG;
    const int rc = occl_check(B, K, Q);
    if (rc) return rc;
    if (workspace_bytes < occl_bwd_bytes(B, K, Q) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return VPN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const OlPlan pl = occl_plan(B, Q);
    float* partial = static_cast<float*>(workspace);
    VPN_LAUNCH(occl_bwd_kernel, dim3(pl.slices, B), dim3(256), 0, st, grad, params, kinds, queries, shared_queries ? 0LL : 3LL * Q,
               labels, labels_u8, lse, s, K, Q, pl.qpl, pl.slices, tau, (double)B * (double)Q, partial);
    const int BK = B * K;                                // <= 65535 * 1024
    VPN_LAUNCH(occl_bwd_finish_kernel, dim3((BK + 3) / 4), dim3(64), 0, st, (const float*)partial, params, BK, K, 4 * pl.slices,
               dparams);
    VPN_LAUNCH_CHECK();
    return 0;
}
