// augment.hip — the batch augmentation stage of train.py:232-237: CutMix of the point clouds and of the images
// (modules/augmentation/cutmix.py) and the gather / interpolation around the auction of point mix-up
// (modules/augmentation/point_mixup.py:24-40).  Nothing here is differentiable: the outputs are data.
//
// Built with -ffp-contract=off: the mix-up interpolation is two rounded products and one rounded sum, as torch
// evaluates (1 - r) * p1 + r * p2.
#include "vpn_common.h"

namespace {

constexpr int CM_THREADS = 1024;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr uint32_t CM_STREAM = 0x80000000u;      // Philox counter word 1: the sampler's streams use the primitive index (< 1024) there

inline int cm_pow2(int v) {
    int p = 64;
    while (p < v) p <<= 1;
    return p;
}
inline int cm_chunks(int N) { return (2 * N + CM_THREADS - 1) / CM_THREADS; }
// 64-bit keys of the 2 N candidates padded to a power of two + one exclusive offset per (chunk, wave) + the total
inline size_t cm_lds_bytes(int N) { return (size_t)cm_pow2(2 * N) * 8 + ((size_t)cm_chunks(N) * CM_WAVES + 1) * 4; }

__device__ inline uint32_t cm_word(uint64_t seed, uint64_t gb, uint32_t slot, uint32_t o[4]) {
    vpn::philox4x32_10(slot, CM_STREAM, (uint32_t)gb, (uint32_t)(gb >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    return o[0];
}

// uniform integer in [0, range) from the four words of one Philox block: multiply-shift with rejection of the low
// products that would favour some values (Lemire 2019); four rejections in a row (probability (range / 2^32)^4) take
// the last word as it is
__device__ inline uint32_t cm_below(const uint32_t o[4], uint32_t range) {
    const uint32_t reject = (0u - range) % range;
    uint32_t hi = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t m = (uint64_t)o[w] * range;
        hi = (uint32_t)(m >> 32);
        if ((uint32_t)m >= reject) break;
    }
    return hi;
}

__device__ inline bool cm_keep(const float* own, const float* par, int N, int cand, float cut) {
    if (cand >= 2 * N) return false;
    return cand < N ? own[(size_t)cand * 3 + 2] >= cut : par[(size_t)(cand - N) * 3 + 2] < cut;     // cutmix.py:32
}

// One workgroup per sample.  Candidates 0..N-1 are the sample's own points, N..2N-1 its partner's; the eligible ones
// are compacted in stable order (ballot + prefix over the waves) into 64-bit keys (Philox word << 32 | candidate), and
//   count > n_out : the n_out smallest keys (bitonic sort in LDS) -- a uniform n_out-subset, in the order of the draw
//   count == n_out: the list as it is
//   0 < count < n_out: n_out independent uniform draws from the list
//   count == 0    : the sample's own first n_out points (the reference raises here; see vpn_hip.h)
__global__ __launch_bounds__(CM_THREADS) void cutmix_points_kernel(
    const float* __restrict__ points, const int32_t* __restrict__ indices, const float* __restrict__ cut_per_sample,
    float cut_all, uint64_t seed, uint64_t sample_base, int B, int N, int n_out, int P, float* __restrict__ out,
    int32_t* __restrict__ src, int32_t* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long cm_keys[];     // [P], then the offsets
    int* woff = reinterpret_cast<int*>(cm_keys + P);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int p = indices ? indices[b] : b;
    if ((unsigned)p >= (unsigned)B) p = b;            // never read outside the batch
    const float cut = cut_per_sample ? cut_per_sample[b] : cut_all;
    const float* own = points + (size_t)b * N * 3;
    const float* par = points + (size_t)p * N * 3;
    const int nchunk = (2 * N + CM_THREADS - 1) / CM_THREADS, E = nchunk * CM_WAVES;
    const uint64_t gb = sample_base + (uint64_t)b;

    for (int k = 0; k < nchunk; ++k) {
        const unsigned long long m = __ballot(cm_keep(own, par, N, k * CM_THREADS + tid, cut));
        if (lane == 0) woff[k * CM_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    if (wave == 0) {                                  // exclusive prefix over the (chunk, wave) counts
        int run = 0;
        for (int base = 0; base < E; base += 64) {
            const int i = base + lane, v = i < E ? woff[i] : 0;
            int inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (i < E) woff[i] = run + inc - v;
            run += __shfl(inc, 63, 64);
        }
        if (lane == 0) woff[E] = run;
    }
    __syncthreads();
    const int cnt = woff[E];
    uint32_t o4[4];
    for (int k = 0; k < nchunk; ++k) {
        const int cand = k * CM_THREADS + tid;
        const bool keep = cm_keep(own, par, N, cand, cut);
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int pos = woff[k * CM_WAVES + wave] + __popcll(m & ((1ull << lane) - 1ull));
            const uint32_t w = cnt > n_out ? cm_word(seed, gb, (uint32_t)pos, o4) : 0u;
            cm_keys[pos] = ((unsigned long long)w << 32) | (uint32_t)cand;
        }
    }
    if (cnt > n_out) {
        int Pc = 64;
        while (Pc < cnt) Pc <<= 1;                    // Pc <= P: cnt <= 2 N
        for (int i = cnt + tid; i < Pc; i += CM_THREADS) cm_keys[i] = ~0ull;
        __syncthreads();
        for (int k = 2; k <= Pc; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < Pc / 2; t += CM_THREADS) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long a = cm_keys[i], c = cm_keys[l];
                    if ((a > c) == ((i & k) == 0)) { cm_keys[i] = c; cm_keys[l] = a; }
                }
                __syncthreads();
            }
        }
    } else {
        __syncthreads();
    }
    for (int i = tid; i < n_out; i += CM_THREADS) {
        int cand;
        if (cnt >= n_out) cand = (int)(uint32_t)cm_keys[i];
        else if (cnt > 0) { cm_word(seed, gb, (uint32_t)i, o4); cand = (int)(uint32_t)cm_keys[cm_below(o4, (uint32_t)cnt)]; }
        else cand = i % N;
        const vpn::F3 v = vpn::ld3(cand < N ? own + (size_t)cand * 3 : par + (size_t)(cand - N) * 3);
        src[(size_t)b * n_out + i] = cand;
        vpn::st3(out + ((size_t)b * n_out + i) * 3, v.x, v.y, v.z);
    }
    if (tid == 0) count[b] = cnt;
}

constexpr int CI_THREADS = 256;

// one thread per float4 of an output row (VEC) or per element; rows [0, rows_a) belong to the first image
template <bool VEC>
__global__ __launch_bounds__(CI_THREADS) void cutmix_images_kernel(
    const float* __restrict__ img_a, const float* __restrict__ img_b, const int32_t* __restrict__ indices, int B,
    int Ca, int Cb, int H, int W, int cut, unsigned total, float* __restrict__ out_a, float* __restrict__ out_b) {
    const unsigned i = blockIdx.x * CI_THREADS + threadIdx.x;
    if (i >= total) return;
    const unsigned per_row = VEC ? W / 4 : W;
    unsigned row = i / per_row;
    const unsigned j = i - row * per_row, rows_a = (unsigned)B * Ca * H;
    const float* in = img_a;
    float* out = out_a;
    unsigned CH = (unsigned)Ca * H;
    if (row >= rows_a) { row -= rows_a; in = img_b; out = out_b; CH = (unsigned)Cb * H; }
    const unsigned b = row / CH, rest = row - b * CH;
    int p = indices[b];
    if ((unsigned)p >= (unsigned)B) p = (int)b;
    const float* self = in + (size_t)row * W;
    const float* part = in + ((size_t)p * CH + rest) * W;
    float* o = out + (size_t)row * W;
    if (VEC) {
        const int x0 = (int)j * 4;
        float4 v;
        if (x0 + 4 <= cut) v = reinterpret_cast<const float4*>(self)[j];
        else if (x0 >= cut) v = reinterpret_cast<const float4*>(part)[j];
        else {
            const float4 s = reinterpret_cast<const float4*>(self)[j], q = reinterpret_cast<const float4*>(part)[j];
            v.x = x0 < cut ? s.x : q.x; v.y = x0 + 1 < cut ? s.y : q.y; v.z = x0 + 2 < cut ? s.z : q.z; v.w = q.w;
        }
        reinterpret_cast<float4*>(o)[j] = v;
    } else {
        o[j] = (int)j < cut ? self[j] : part[j];
    }
}

constexpr int MX_THREADS = 256;

__global__ __launch_bounds__(MX_THREADS) void mixup_gather_kernel(const float* __restrict__ points,
                                                                  const int32_t* __restrict__ indices, int B, int n,
                                                                  unsigned total, float* __restrict__ out) {
    const unsigned i = blockIdx.x * MX_THREADS + threadIdx.x;
    if (i >= total) return;
    const unsigned b = i / (unsigned)n, r = i - b * (unsigned)n;
    int p = indices[b];
    if ((unsigned)p >= (unsigned)B) p = (int)b;
    const vpn::F3 v = vpn::ld3(points + ((size_t)p * n + r) * 3);
    vpn::st3(out + (size_t)i * 3, v.x, v.y, v.z);
}

__global__ __launch_bounds__(MX_THREADS) void mixup_lerp_kernel(const float* __restrict__ points,
                                                                const float* __restrict__ partner,
                                                                const int32_t* __restrict__ assignment, int n,
                                                                unsigned total, float wa, float wb,
                                                                float* __restrict__ out) {
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * MX_THREADS + threadIdx.x;
    if (i >= total) return;
    const unsigned b = i / (unsigned)n;
    const int j = assignment[i];
    vpn::F3 x = vpn::ld3(points + (size_t)i * 3);
    if ((unsigned)j < (unsigned)n) {                 // an unassigned point (-1) keeps its own position
        const vpn::F3 y = vpn::ld3(partner + ((size_t)b * n + j) * 3);
        x.x = wa * x.x + wb * y.x;
        x.y = wa * x.y + wb * y.y;
        x.z = wa * x.z + wb * y.z;
    }
    vpn::st3(out + (size_t)i * 3, x.x, x.y, x.z);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" size_t vpn_cutmix_points_lds(int N) {
    if (N <= 0 || N > VPN_CUTMIX_MAX_POINTS) return 0;
    return cm_lds_bytes(N);
}

extern "C" int vpn_cutmix_points(const float* points, const int32_t* indices, const float* cut_per_sample, float cut,
                                 uint64_t seed, uint64_t sample_base, int B, int N, int n_out, float* out,
                                 int32_t* src, int32_t* count, void* stream) {
    if (!points || !out || !src || !count || B <= 0 || N <= 0 || n_out <= 0) return VPN_E_BADARG;
    if (N > VPN_CUTMIX_MAX_POINTS || n_out > 2 * VPN_CUTMIX_MAX_POINTS) return VPN_E_TOOBIG;      // before any HIP call
    hipStream_t s = (hipStream_t)stream;
    static size_t raised = 65536;
    const size_t lds = cm_lds_bytes(N);
    if (lds > raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cutmix_points_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)cm_lds_bytes(VPN_CUTMIX_MAX_POINTS));
        if (e != hipSuccess) return (int)e;
        raised = cm_lds_bytes(VPN_CUTMIX_MAX_POINTS);
    }
    VPN_LAUNCH(cutmix_points_kernel, dim3(B), dim3(CM_THREADS), lds, s, points, indices, cut_per_sample, cut, seed,
               sample_base, B, N, n_out, cm_pow2(2 * N), out, src, count);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_cutmix_images(const float* img_a, const float* img_b, const int32_t* indices, int B, int Ca, int Cb,
                                 int H, int W, int cut_index, float* out_a, float* out_b, void* stream) {
    if (!img_a || !out_a || !indices || B <= 0 || Ca <= 0 || Cb < 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    if (Cb > 0 && (!img_b || !out_b)) return VPN_E_BADARG;
    if (cut_index < 0 || cut_index > W) return VPN_E_BADARG;
    const bool vec = W % 4 == 0 && aligned16(img_a) && aligned16(out_a) && (Cb == 0 || (aligned16(img_b) && aligned16(out_b)));
    const uint64_t total = (uint64_t)B * (Ca + Cb) * H * (vec ? W / 4 : W);
    if (total > 0x7fffffffull || (uint64_t)B * (Ca + Cb) * H * W > 0x7fffffffull) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((total + CI_THREADS - 1) / CI_THREADS));
    if (vec)
        VPN_LAUNCH_AS("cutmix_images_kernel", cutmix_images_kernel<true>, grid, dim3(CI_THREADS), 0, s, img_a, img_b,
                      indices, B, Ca, Cb, H, W, cut_index, (unsigned)total, out_a, out_b);
    else
        VPN_LAUNCH_AS("cutmix_images_kernel", cutmix_images_kernel<false>, grid, dim3(CI_THREADS), 0, s, img_a, img_b,
                      indices, B, Ca, Cb, H, W, cut_index, (unsigned)total, out_a, out_b);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_mixup_gather(const float* points, const int32_t* indices, int B, int n, float* out, void* stream) {
    if (!points || !indices || !out || B <= 0 || n <= 0) return VPN_E_BADARG;
    const uint64_t total = (uint64_t)B * n;
    if (total * 3 > 0x7fffffffull) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(mixup_gather_kernel, dim3((unsigned)((total + MX_THREADS - 1) / MX_THREADS)), dim3(MX_THREADS), 0, s,
               points, indices, B, n, (unsigned)total, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_mixup_lerp(const float* points, const float* partner, const int32_t* assignment, int B, int n,
                              float wa, float wb, float* out, void* stream) {
    if (!points || !partner || !assignment || !out || B <= 0 || n <= 0) return VPN_E_BADARG;
    const uint64_t total = (uint64_t)B * n;
    if (total * 3 > 0x7fffffffull) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(mixup_lerp_kernel, dim3((unsigned)((total + MX_THREADS - 1) / MX_THREADS)), dim3(MX_THREADS), 0, s,
               points, partner, assignment, n, (unsigned)total, wa, wb, out);
    VPN_LAUNCH_CHECK();
    return 0;
}
