// surfeval.hip — surface evaluation: the metrics single-view reconstruction reports on points sampled from
// the predicted SURFACE -- Chamfer-L2 and -L1, precision / recall / F-score at distance thresholds, normal consistency -- per
// sample, and the per-class bookkeeping of an evaluation epoch, on the device.  The expensive parts exist already (the
// area-weighted sampler with its face indices, the nearest-neighbour scan with indices both ways); this file holds the step
// from face indices to unit normals, the per-sample row and the bookkeeping.
//
//   surfeval_normals_kernel   one work-item per (sample, point): face index -> unit normal, batched or ragged layout
//   surfeval_sample_kernel    one workgroup per sample: the row of W = 6 + 3 T values (include/vpn_hip.h lists the columns)
//   surfeval_book_kernel      ONE workgroup, launched after the sample kernel on the same stream: state += the batch
//
// No atomics, no scratch, no hand-off between workgroups: the second launch sees the rows because it is a later launch on
// the same stream.  Every floating sum has one fixed order, so the results are bit-equal from run to run.
//
// State (vpn_surfeval_state_size), zeroed by the caller, W = 6 + 3 T:
//   doubles  total[W]  class_sum[C][W]          int64  n_samples  n_batches  n_invalid  class_n[C]
//
// Built with -ffp-contract=off: every product and sum below is rounded by itself, in fp32 for the normals and in fp64 for
// the sums, whatever the compiler would contract.
#include "vpn_common.h"
#include <float.h>

namespace {

constexpr int SE_T = VPN_SURFEVAL_MAX_THRESHOLDS;
constexpr int SE_W = 6 + 3 * SE_T;       // the widest row
constexpr int SE_CHUNK = 128;            // samples of a batch the bookkeeping stages in LDS at a time
constexpr int SE_MAX_ITEMS = VPN_SURFEVAL_MAX_ITEMS;    // N, M, n, P, F, sumP, sumF, C

inline size_t se_doubles(int C, int T) { return (1 + (size_t)C) * (size_t)(6 + 3 * T); }
inline size_t se_counts(int C) { return 3 + (size_t)C; }

// the affine rows of view_center_xforms / genre_xforms, summed the way ragged_sample_kernel maps its points
__device__ inline vpn::F3 se_map(const float* __restrict__ m, vpn::F3 v) {
    return vpn::F3{m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3], m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7],
                   m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11]};
}

// Batched layout (vert_offset == NULL): verts [B,P,3], faces [F,3], fidx [B,n].  Ragged layout: verts [P,3] (P = sumP), faces
// [F,3] mesh-local (F = sumF), sample b belongs to mesh b / sets.  xforms [B,3,4] in both (B = S sets in the ragged one).
__global__ __launch_bounds__(256) void surfeval_normals_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ vert_offset,
                                                               const int32_t* __restrict__ face_offset,
                                                               const int32_t* __restrict__ fidx, const float* __restrict__ xforms,
                                                               int n, int P, int F, int sets, float* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long vbase, nv, fbase, nf;
    if (vert_offset) {
        const int s = b / sets;
        vbase = vert_offset[s]; nv = (long long)vert_offset[s + 1] - vbase;
        fbase = face_offset[s]; nf = (long long)face_offset[s + 1] - fbase;
        // a table that does not describe the packed arrays names no vertex and no face
        if (vbase < 0 || nv < 0 || vbase + nv > P) nv = 0;
        if (fbase < 0 || nf < 0 || fbase + nf > F) nf = 0;
    } else {
        vbase = (long long)b * P; nv = P; fbase = 0; nf = F;
    }
    const size_t o = (size_t)b * n + i;
    const long long f = fidx[o];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (f >= 0 && f < nf) {
        const int32_t* fc = faces + (size_t)(fbase + f) * 3;
        const long long i0 = fc[0], i1 = fc[1], i2 = fc[2];
        if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
            vpn::F3 a = vpn::ld3(verts + (size_t)(vbase + i0) * 3), p = vpn::ld3(verts + (size_t)(vbase + i1) * 3),
                    q = vpn::ld3(verts + (size_t)(vbase + i2) * 3);
            if (xforms) {
                const float* m = xforms + (size_t)b * 12;      // the same 12 values for every point of the sample
                a = se_map(m, a); p = se_map(m, p); q = se_map(m, q);
            }
            const float e1x = p.x - a.x, e1y = p.y - a.y, e1z = p.z - a.z;
            const float e2x = q.x - a.x, e2y = q.y - a.y, e2z = q.z - a.z;
            const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
            const float cc = cx * cx + cy * cy + cz * cz;
            if (cc > 0.0f && cc <= FLT_MAX) {                   // not 0, not inf, not NaN
                const float l = sqrtf(cc);
                nx = cx / l; ny = cy / l; nz = cz / l;
            }
        }
    }
    vpn::st3(out + o * 3, nx, ny, nz);
}

__device__ inline int clamp_index(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

// One direction of one sample in this lane's elements t, t + 256, ...: the sums of d^2, d and |na . nb[idx]| in fp64 and the
// threshold counts.  dist is what the nearest-neighbour scan writes: the Euclidean distance, NOT squared (the reference's
// Chamfer takes the root, chamfer_distance.py:14-23).  Its square is formed in fp64, where the product of two fp32 values
// is exact, so neither the squared mean nor a threshold decision depends on a rounding or a build flag.
__device__ inline void se_direction(const float* __restrict__ dist, const int32_t* __restrict__ idx, const float* __restrict__ na,
                                    const float* __restrict__ nb, int n, int n_other, const double thr[SE_T], int tid, double& s2,
                                    double& s1, double& snc, int cnt[SE_T]) {
    for (int i = tid; i < n; i += 256) {
        const double d = (double)dist[i];
        const double q = d * d;
        s2 += q;
        s1 += d;
#pragma unroll
        for (int t = 0; t < SE_T; ++t) cnt[t] += q < thr[t];               // a NaN distance is a miss
        if (na) {
            const int j = clamp_index(idx[i], n_other);
            const vpn::F3 a = vpn::ld3(na + (size_t)i * 3), c = vpn::ld3(nb + (size_t)j * 3);
            const double dot = (double)a.x * (double)c.x + (double)a.y * (double)c.y + (double)a.z * (double)c.z;
            snc += fabs(dot);
        }
    }
}

// One workgroup (256 lanes) per sample.  Lane t owns elements t, t + 256, ...; xor tree over the wave; the four waves in
// order; divided and rounded to fp32 once.  Counts are integers and exact; P, R and F are formed in fp64 from them.
__global__ __launch_bounds__(256) void surfeval_sample_kernel(const float* __restrict__ d1, const int32_t* __restrict__ i1,
                                                              const float* __restrict__ d2, const int32_t* __restrict__ i2,
                                                              const float* __restrict__ n_pred, const float* __restrict__ n_gt,
                                                              const float* __restrict__ thr2, int N, int M, int T,
                                                              float* __restrict__ per_sample) {
    __shared__ double dred[4][6];
    __shared__ int cred[4][2 * SE_T];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double thr[SE_T];
#pragma unroll
    for (int t = 0; t < SE_T; ++t) thr[t] = t < T ? (double)thr2[t] : 0.0;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};             // acc2 comp2 acc1 comp1 nc1 nc2
    int c1[SE_T], c2[SE_T];
#pragma unroll
    for (int t = 0; t < SE_T; ++t) c1[t] = c2[t] = 0;
    const bool normals = n_pred != nullptr;
    se_direction(d1 + (size_t)b * N, i1 + (size_t)b * N, normals ? n_pred + (size_t)b * N * 3 : nullptr,
                 normals ? n_gt + (size_t)b * M * 3 : nullptr, N, M, thr, tid, s[0], s[2], s[4], c1);
    se_direction(d2 + (size_t)b * M, i2 + (size_t)b * M, normals ? n_gt + (size_t)b * M * 3 : nullptr,
                 normals ? n_pred + (size_t)b * N * 3 : nullptr, M, N, thr, tid, s[1], s[3], s[5], c2);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
    }
#pragma unroll
    for (int t = 0; t < SE_T; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { c1[t] += __shfl_xor(c1[t], o, 64); c2[t] += __shfl_xor(c2[t], o, 64); }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) dred[wave][k] = s[k];
#pragma unroll
        for (int t = 0; t < SE_T; ++t) { cred[wave][t] = c1[t]; cred[wave][SE_T + t] = c2[t]; }
    }
    __syncthreads();
    float* row = per_sample + (size_t)b * (6 + 3 * T);
    if (tid < 6) {
        const double sum = (dred[0][tid] + dred[1][tid]) + (dred[2][tid] + dred[3][tid]);
        row[tid] = (float)(sum / (double)((tid & 1) ? M : N));
    } else if (tid >= 64 && tid < 64 + T) {
        const int t = tid - 64;
        const int np = (cred[0][t] + cred[1][t]) + (cred[2][t] + cred[3][t]);
        const int nr = (cred[0][SE_T + t] + cred[1][SE_T + t]) + (cred[2][SE_T + t] + cred[3][SE_T + t]);
        const double p = (double)np / (double)N, r = (double)nr / (double)M;
        row[6 + t] = (float)p;
        row[6 + T + t] = (float)r;
        row[6 + 2 * T + t] = p + r > 0.0 ? (float)(2.0 * p * r / (p + r)) : 0.0f;
    }
}

// ONE workgroup.  Work-item j < (1 + C) W owns (group j / W, column j % W), strided by 256: group 0 is the total over ALL
// samples, group 1 + c is class c.  It walks the samples in order b = 0 .. B-1, which is the order Python's `+= float(x)`
// adds in, so the state is bit-equal to a host loop over the rows.  Lane c owns class_n[c]; lane 255 the three counts.
__global__ __launch_bounds__(256) void surfeval_book_kernel(const float* __restrict__ per_sample,
                                                            const int32_t* __restrict__ class_index, int B, int C, int W,
                                                            double* __restrict__ state) {
    __shared__ float s_row[SE_CHUNK * SE_W];
    __shared__ int s_cls[SE_CHUNK];
    const int tid = threadIdx.x;
    const int items = (1 + C) * W;
    long long* counts = reinterpret_cast<long long*>(state + (size_t)items);
    long long invalid = 0;
    for (int base = 0; base < B; base += SE_CHUNK) {
        const int m = min(SE_CHUNK, B - base);
        __syncthreads();                                 // the previous chunk has been read
        for (int i = tid; i < m * W; i += 256) s_row[i] = per_sample[(size_t)base * W + i];
        for (int i = tid; i < m; i += 256) s_cls[i] = class_index[base + i];
        __syncthreads();
        for (int j = tid; j < items; j += 256) {
            const int g = j / W, k = j - g * W;
            double a = state[j];
            for (int i = 0; i < m; ++i) {
                if (g == 0 || s_cls[i] == g - 1) a += (double)s_row[i * W + k];
            }
            state[j] = a;
        }
        for (int c = tid; c < C; c += 256) {
            long long k = counts[3 + c];
            for (int i = 0; i < m; ++i) k += s_cls[i] == c;
            counts[3 + c] = k;
        }
        if (tid == 255) {
            for (int i = 0; i < m; ++i) invalid += (unsigned)s_cls[i] >= (unsigned)C;
        }
    }
    if (tid == 255) {
        counts[0] += B;
        counts[1] += 1;
        counts[2] += invalid;
    }
}

}  // namespace

extern "C" size_t vpn_surfeval_state_size(int num_classes, int T) {
    if (num_classes <= 0 || num_classes > SE_MAX_ITEMS || T < 1 || T > SE_T) return 0;
    return (se_doubles(num_classes, T) + se_counts(num_classes)) * 8;
}

extern "C" int vpn_face_normals_at(const float* verts, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                                   const int32_t* fidx, const float* xforms, int B, int n, int P, int F, int sets, float* normals,
                                   void* stream) {
    if (!verts || !faces || !fidx || !normals) return VPN_E_BADARG;
    if ((vert_offset == nullptr) != (face_offset == nullptr)) return VPN_E_BADARG;
    if (B <= 0 || n <= 0 || P <= 0 || F <= 0 || sets <= 0) return VPN_E_BADARG;
    if (vert_offset && B % sets) return VPN_E_BADARG;            // the ragged layout has S sets samples
    if (B > 65535 || n > SE_MAX_ITEMS || P > SE_MAX_ITEMS || F > SE_MAX_ITEMS) return VPN_E_TOOBIG;
    VPN_LAUNCH(surfeval_normals_kernel, dim3((n + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, verts, faces, vert_offset,
               face_offset, fidx, xforms, n, P, F, sets, normals);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_surfeval_accumulate(const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2,
                                       const float* n_pred, const float* n_gt, const float* thr2, const int32_t* class_index, int B,
                                       int N, int M, int T, int num_classes, void* state, float* per_sample, void* stream) {
    if (!dist1 || !idx1 || !dist2 || !idx2 || !thr2 || !class_index || !state || !per_sample) return VPN_E_BADARG;
    if ((n_pred == nullptr) != (n_gt == nullptr)) return VPN_E_BADARG;
    if (B <= 0 || N <= 0 || M <= 0 || T <= 0 || num_classes <= 0) return VPN_E_BADARG;
    if (reinterpret_cast<uintptr_t>(state) & 7) return VPN_E_BADARG;
    if (T > SE_T || B > 65535 || N > SE_MAX_ITEMS || M > SE_MAX_ITEMS || num_classes > SE_MAX_ITEMS) return VPN_E_TOOBIG;
    VPN_LAUNCH(surfeval_sample_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, dist1, idx1, dist2, idx2, n_pred, n_gt, thr2, N,
               M, T, per_sample);
    VPN_LAUNCH_CHECK();
    VPN_LAUNCH(surfeval_book_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)per_sample, class_index, B,
               num_classes, 6 + 3 * T, static_cast<double*>(state));
    VPN_LAUNCH_CHECK();
    return 0;
}
