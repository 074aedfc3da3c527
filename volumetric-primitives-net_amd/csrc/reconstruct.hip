// reconstruct.hip — cloud -> mesh of ONE topology for a whole batch, on the device: the step between
// mixup_points and the Phong render of point_mixup.py:12-21.  The reference reconstructs a surface by ball pivoting
// (open3d) and decomposes it with V-HACD (an external binary), per sample, on the host; here a cloud is split into H
// clusters (farthest-point seeds + Lloyd rounds) and every cluster becomes the polytope of its support points along D
// fixed directions.  Every decision is an arg-max / arg-min with a stated tie rule, every centre an exact integer mean,
// so tests/reconstruct_ref.py pins the outputs bit for bit.  Nothing here is differentiable: the outputs are data.
//
// Built with -ffp-contract=off: squared distances and support values are rounded per operation, summed x, y, z.
#include "vpn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CL_THREADS = 1024;
constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr float RC_FIX = 1048576.0f;            // 2^20: the fixed-point scale of the integer means
constexpr double RC_FIX_D = 1048576.0;

typedef unsigned long long u64;

// x, y, z and the running seed distance of every point (SoA: lane i reads word i, no bank conflicts)
inline size_t cl_lds_bytes(int n) { return (size_t)n * 16; }
// the members of one cluster, compacted: x, y, z and the point index
inline size_t sh_lds_bytes(int n) { return (size_t)n * 16; }

__device__ inline float rc_dist2(float px, float py, float pz, float cx, float cy, float cz) {
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline long long rc_fix(float v) { return (long long)rintf(v * RC_FIX); }      // exact scaling, ties to even

__device__ inline float rc_mean(long long sum, int count) { return (float)((double)sum / ((double)count * RC_FIX_D)); }

__device__ inline long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// (value bits, inverted index): the largest key is the largest non-negative value, the lowest index among equals
__device__ inline u64 rc_key(float v, int i) { return ((u64)__float_as_uint(v) << 32) | (0xffffffffu - (uint32_t)i); }
__device__ inline int rc_key_index(u64 k) { return (int)(0xffffffffu - (uint32_t)k); }

// One workgroup per sample.  Integer sums go through 64-bit LDS atomics (exact in any order); the arg-max of a seed
// step through one 64-bit LDS max per wave.
__global__ __launch_bounds__(CL_THREADS) void cluster_points_kernel(const float* __restrict__ points, int n, int H,
                                                                    int iters, int32_t* __restrict__ labels,
                                                                    float* __restrict__ centres,
                                                                    int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) float cl_lds[];
    float* X = cl_lds;
    float* Y = X + n;
    float* Z = Y + n;
    float* mind = Z + n;
    __shared__ long long sums[VPN_CLUSTER_MAX_HULLS][3];
    __shared__ int cnt[VPN_CLUSTER_MAX_HULLS];
    __shared__ float C[VPN_CLUSTER_MAX_HULLS][3];
    __shared__ u64 best[VPN_CLUSTER_MAX_HULLS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float* P = points + (size_t)b * n * 3;

    if (tid < VPN_CLUSTER_MAX_HULLS) {
        sums[tid][0] = sums[tid][1] = sums[tid][2] = 0;
        cnt[tid] = 0;
        best[tid] = 0ull;
    }
    __syncthreads();
    {   // the cloud into LDS and its integer sums into sums[0] (cleared again after seed 0)
        long long sx = 0, sy = 0, sz = 0;
        for (int i = tid; i < n; i += CL_THREADS) {
            const vpn::F3 p = vpn::ld3(P + (size_t)i * 3);
            X[i] = p.x; Y[i] = p.y; Z[i] = p.z;
            sx += rc_fix(p.x); sy += rc_fix(p.y); sz += rc_fix(p.z);
        }
        sx = wave_sum_i64(sx); sy = wave_sum_i64(sy); sz = wave_sum_i64(sz);
        if (lane == 0) {
            atomicAdd(reinterpret_cast<u64*>(&sums[0][0]), (u64)sx);
            atomicAdd(reinterpret_cast<u64*>(&sums[0][1]), (u64)sy);
            atomicAdd(reinterpret_cast<u64*>(&sums[0][2]), (u64)sz);
        }
    }
    __syncthreads();
    const float mx = rc_mean(sums[0][0], n), my = rc_mean(sums[0][1], n), mz = rc_mean(sums[0][2], n);
    {   // seed 0: the point farthest from the mean
        u64 k = 0ull;
        for (int i = tid; i < n; i += CL_THREADS) {
            const u64 c = rc_key(rc_dist2(X[i], Y[i], Z[i], mx, my, mz), i);
            k = c > k ? c : k;
        }
        k = wave_max_u64(k);
        if (lane == 0) atomicMax(&best[0], k);
    }
    __syncthreads();
    if (tid < 3) sums[0][tid] = 0;
    for (int s = 1; s <= H; ++s) {              // step s: fold seed s - 1 into the running minimum, pick seed s
        const int j = rc_key_index(best[s - 1]);
        const float cx = X[j], cy = Y[j], cz = Z[j];
        if (tid == 0) { C[s - 1][0] = cx; C[s - 1][1] = cy; C[s - 1][2] = cz; }
        if (s == H) break;
        u64 k = 0ull;
        for (int i = tid; i < n; i += CL_THREADS) {
            float d = rc_dist2(X[i], Y[i], Z[i], cx, cy, cz);
            if (s > 1) d = fminf(mind[i], d);
            mind[i] = d;
            const u64 c = rc_key(d, i);
            k = c > k ? c : k;
        }
        k = wave_max_u64(k);
        if (lane == 0) atomicMax(&best[s], k);
        __syncthreads();
    }
    __syncthreads();

    for (int it = 0; it <= iters; ++it) {       // `iters` Lloyd rounds, then the final assignment
        const bool last = it == iters;
        for (int i = tid; i < n; i += CL_THREADS) {
            const float px = X[i], py = Y[i], pz = Z[i];
            float bd = rc_dist2(px, py, pz, C[0][0], C[0][1], C[0][2]);
            int bh = 0;
            for (int h = 1; h < H; ++h) {
                const float d = rc_dist2(px, py, pz, C[h][0], C[h][1], C[h][2]);
                if (d < bd) { bd = d; bh = h; }                     // equal distances stay with the lowest centre
            }
            atomicAdd(&cnt[bh], 1);
            if (last) {
                labels[(size_t)b * n + i] = bh;
            } else {
                atomicAdd(reinterpret_cast<u64*>(&sums[bh][0]), (u64)rc_fix(px));
                atomicAdd(reinterpret_cast<u64*>(&sums[bh][1]), (u64)rc_fix(py));
                atomicAdd(reinterpret_cast<u64*>(&sums[bh][2]), (u64)rc_fix(pz));
            }
        }
        __syncthreads();
        if (tid < H) {
            const int c = cnt[tid];
            if (last) {
                counts[(size_t)b * H + tid] = c;
                vpn::st3(centres + ((size_t)b * H + tid) * 3, C[tid][0], C[tid][1], C[tid][2]);
            } else {
                if (c > 0) {                                        // an empty cluster keeps its centre
                    C[tid][0] = rc_mean(sums[tid][0], c);
                    C[tid][1] = rc_mean(sums[tid][1], c);
                    C[tid][2] = rc_mean(sums[tid][2], c);
                }
                sums[tid][0] = sums[tid][1] = sums[tid][2] = 0;
                cnt[tid] = 0;
            }
        }
        __syncthreads();
    }
}

// One workgroup per (cluster, sample).  The members are compacted into LDS in index order (each wave owns a contiguous
// range of the cloud: count, prefix over the waves, write), then one thread per direction walks them: all lanes read the
// same member (an LDS broadcast), `>` keeps the first of equal values, which is the lowest point index.
__global__ __launch_bounds__(SH_THREADS) void support_hulls_kernel(const float* __restrict__ points,
                                                                   const int32_t* __restrict__ labels,
                                                                   const float* __restrict__ centres,
                                                                   const float* __restrict__ dirs, int n, int H, int D,
                                                                   float* __restrict__ verts,
                                                                   int32_t* __restrict__ support) {
    extern __shared__ __attribute__((aligned(16))) float sh_lds[];
    float* X = sh_lds;
    float* Y = X + n;
    float* Z = Y + n;
    int* I = reinterpret_cast<int*>(Z + n);
    __shared__ int woff[SH_WAVES + 1];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* P = points + (size_t)b * n * 3;
    const int32_t* L = labels + (size_t)b * n;
    const int per = ((n + SH_WAVES - 1) / SH_WAVES + 63) & ~63;     // points per wave, whole rounds of 64
    const int lo = wave * per, hi = min(n, lo + per);

    int mine = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        mine += __popcll(__ballot(i < hi && L[i] == h));
    }
    if (lane == 0) woff[wave] = mine;
    __syncthreads();
    int off = 0, m = 0;
#pragma unroll
    for (int w = 0; w < SH_WAVES; ++w) {
        const int c = woff[w];
        if (w < wave) off += c;
        m += c;
    }
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool in = i < hi && L[i] == h;
        const u64 mask = __ballot(in);
        if (in) {
            const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));     // pos < m <= n
            const vpn::F3 p = vpn::ld3(P + (size_t)i * 3);
            X[pos] = p.x; Y[pos] = p.y; Z[pos] = p.z; I[pos] = i;
        }
        off += __popcll(mask);
    }
    __syncthreads();

    const size_t row = ((size_t)b * H + h) * D;
    if (m == 0) {                                                   // an empty cluster: D copies of its centre
        const vpn::F3 c = vpn::ld3(centres + ((size_t)b * H + h) * 3);
        for (int d = tid; d < D; d += SH_THREADS) {
            vpn::st3(verts + (row + d) * 3, c.x, c.y, c.z);
            support[row + d] = -1;
        }
        return;
    }
    for (int d = tid; d < D; d += SH_THREADS) {
        const vpn::F3 dir = vpn::ld3(dirs + (size_t)d * 3);
        float bv = (X[0] * dir.x + Y[0] * dir.y) + Z[0] * dir.z;
        int bj = 0;
        for (int j = 1; j < m; ++j) {
            const float v = (X[j] * dir.x + Y[j] * dir.y) + Z[j] * dir.z;
            if (v > bv) { bv = v; bj = j; }
        }
        vpn::st3(verts + (row + d) * 3, X[bj], Y[bj], Z[bj]);
        support[row + d] = I[bj];
    }
}

// dynamic LDS above the default limit has to be allowed for the kernel on the CURRENT device: asked for on every call
// that needs it (no per-process mark, which another device or another host thread would not share)
template <typename K>
inline int rc_allow_lds(K kernel, size_t need, size_t most) {
    if (need <= 49152) return 0;                // the static arrays of the kernels share the default 64 KiB
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
}

}  // namespace

extern "C" int vpn_cluster_points(const float* points, int B, int n, int H, int iters, int32_t* labels, float* centres,
                                  int32_t* counts, void* stream) {
    if (!points || !labels || !centres || !counts || B <= 0 || n <= 0 || H <= 0 || iters < 0) return VPN_E_BADARG;
    if (n > VPN_CLUSTER_MAX_POINTS || H > VPN_CLUSTER_MAX_HULLS || B > 65535) return VPN_E_TOOBIG;     // before any HIP call
    hipStream_t s = (hipStream_t)stream;
    const int rc = rc_allow_lds(cluster_points_kernel, cl_lds_bytes(n), cl_lds_bytes(VPN_CLUSTER_MAX_POINTS));
    if (rc) return rc;
    VPN_LAUNCH(cluster_points_kernel, dim3(B), dim3(CL_THREADS), cl_lds_bytes(n), s, points, n, H, iters, labels, centres, counts);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_support_hulls(const float* points, const int32_t* labels, const float* centres, const float* dirs, int B,
                                 int n, int H, int D, float* verts, int32_t* support, void* stream) {
    if (!points || !labels || !centres || !dirs || !verts || !support || B <= 0 || n <= 0 || H <= 0 || D <= 0) return VPN_E_BADARG;
    if (n > VPN_CLUSTER_MAX_POINTS || H > VPN_CLUSTER_MAX_HULLS || B > 65535 || (uint64_t)B * H * D * 3 > 0x7fffffffull) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    const int rc = rc_allow_lds(support_hulls_kernel, sh_lds_bytes(n), sh_lds_bytes(VPN_CLUSTER_MAX_POINTS));
    if (rc) return rc;
    VPN_LAUNCH(support_hulls_kernel, dim3(H, B), dim3(SH_THREADS), sh_lds_bytes(n), s, points, labels, centres, dirs, n, H, D, verts, support);
    VPN_LAUNCH_CHECK();
    return 0;
}
