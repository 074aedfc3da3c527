// acdmix.hip — the middle of the ACD-mix stage: the hulls of two objects are augmented per object
// (acd.py:31-77,114-119) and merged (generate.py:140-148).  The reference merges with trimesh.boolean.union on the host;
// here the SURFACE of the union is sampled instead: candidates drawn on all augmented hulls survive unless they lie inside
// another kept hull, where "inside" is decided on the outer polytope of a hull along the template's directions.  Every
// decision is a comparison of values rounded per operation, so tests/acdmix_ref.py pins the outputs bit for bit.
// Nothing here is differentiable: the outputs are data.
//
// Built with -ffp-contract=off: dot(p, d) = (px dx + py dy) + pz dz, every operation rounded by itself.
#include "vpn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int HA_THREADS = 256;
constexpr int HA_WAVES = HA_THREADS / 64;
constexpr int US_THREADS = 1024;
constexpr int US_WAVES = US_THREADS / 64;
constexpr int US_MAX_CHUNKS = (VPN_UNION_MAX_CAND + US_THREADS - 1) / US_THREADS;      // one flag bit per chunk and thread
static_assert(US_MAX_CHUNKS <= 32, "the survivor flags of a thread live in one 32-bit word");
static_assert(VPN_UNION_MAX_HULLS <= 64, "one lane per hull in the cut-out");

typedef unsigned long long u64;

__device__ inline float am_dot(float px, float py, float pz, float dx, float dy, float dz) {
    return (px * dx + py * dy) + pz * dz;
}

// One workgroup per (object, sample).  Wave w looks at hulls w, w + 4, ...: three ballots over a hull's D vertices are
// is_center (acd.py:31-34; min |z| < 0.05 is "some |z| < 0.05").  Lane g of wave 0 then decides hull g: its rank among the
// centre hulls by (u_hull, index) against the number to cut.  Object 0's workgroup also collapses the hulls that belong
// to no object, so every element of out / keep is written.
__global__ __launch_bounds__(HA_THREADS) void hull_augment_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ group, const int32_t* __restrict__ coin,
    const float* __restrict__ u_num, const float* __restrict__ scale, const int32_t* __restrict__ turn,
    const float* __restrict__ shift, const float* __restrict__ u_hull, int G, int D, int O, float* __restrict__ out,
    int32_t* __restrict__ keep) {
    __shared__ int centre[VPN_UNION_MAX_HULLS];
    __shared__ int kept[VPN_UNION_MAX_HULLS];
    const int o = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* V = verts + (size_t)s * G * D * 3;
    float* W = out + (size_t)s * G * D * 3;

    for (int g = wave; g < G; g += HA_WAVES) {
        if (group[g] != o) continue;                    // uniform over the wave
        bool pos = false, neg = false, nz = false;
        for (int d = lane; d < D; d += 64) {
            const float z = V[((size_t)g * D + d) * 3 + 2];
            pos |= z > 0.0f;
            neg |= z < 0.0f;
            nz |= fabsf(z) < 0.05f;
        }
        const bool c = (__ballot(pos) != 0ull && __ballot(neg) != 0ull) || __ballot(nz) != 0ull;
        if (lane == 0) centre[g] = c ? 1 : 0;
    }
    __syncthreads();
    if (wave == 0) {
        const int g = lane;
        const int grp = g < G ? group[g] : -1;
        const bool member = g < G && grp == o;
        const bool c = member && centre[g] != 0;
        const int nC = __popcll(__ballot(c));
        const size_t so = (size_t)s * O + o;
        const float key = g < G ? u_hull[(size_t)s * G + g] : 0.0f;
        int rank = 0;
        for (int j = 0; j < G; ++j) {                   // G <= 64: every lane sees every hull
            const float kj = __shfl(key, j, 64);
            const bool cj = __shfl((int)c, j, 64) != 0;
            rank += (cj && (kj < key || (kj == key && j < g))) ? 1 : 0;
        }
        bool k;
        if (nC == 0) {
            k = member;                                 // THE DEVIATION: no centre hull keeps the object as it is
        } else if (coin[so] != 0 && nC > 1) {           // acd.py:70-73
            const float t = fminf(fmaxf(floorf(u_num[so] * (float)(nC - 1)), 0.0f), (float)(nC - 2));
            const int ncut = 1 + (int)t;                // 1 .. nC - 1
            k = member && !(c && rank < ncut);
        } else {
            k = c;                                      // acd.py:75
        }
        if (g < G) {
            kept[g] = k ? 1 : 0;
            if (member) keep[(size_t)s * G + g] = k ? 1 : 0;
            else if (o == 0 && (unsigned)grp >= (unsigned)O) keep[(size_t)s * G + g] = 0;
        }
    }
    __syncthreads();
    const size_t so = (size_t)s * O + o;
    const float sc = scale[so], sh = shift[so];
    const int tn = turn[so];
    for (int g = 0; g < G; ++g) {
        const int grp = group[g];
        const bool member = grp == o, stray = o == 0 && (unsigned)grp >= (unsigned)O;
        if (!member && !stray) continue;
        const float* src = V + (size_t)g * D * 3;
        float* dst = W + (size_t)g * D * 3;
        if (stray || kept[g] == 0) {                    // a cut hull: D copies of its first vertex, zero-area faces
            const vpn::F3 p = vpn::ld3(src);
            for (int d = tid; d < D; d += HA_THREADS) vpn::st3(dst + (size_t)d * 3, p.x, p.y, p.z);
            continue;
        }
        for (int d = tid; d < D; d += HA_THREADS) {
            const vpn::F3 p = vpn::ld3(src + (size_t)d * 3);
            const float x = p.x * sc, y = p.y * sc, z = p.z * sc;             // acd.py:41
            float rx, ry;                                                      // acd.py:59-62, R(angle) about +z
            switch (tn) {
                case 0: rx = -y; ry = x; break;                                //  90: (x, y) -> (-y,  x)
                case 1: rx = y; ry = -x; break;                                // -90: (x, y) -> ( y, -x)
                case 3: case 4: rx = -x; ry = -y; break;                       // 180, -180: (x, y) -> (-x, -y)
                default: rx = x; ry = y; break;                                //   0 (and any index outside 0..4)
            }
            vpn::st3(dst + (size_t)d * 3, rx, ry + sh, z);                     // acd.py:50
        }
    }
}

// dirs as (x, y, z, 0) and the support values of all hulls, then the survivor list
inline size_t us_lds_bytes(int G, int D, int nc) { return ((size_t)D * 4 + (size_t)G * D + (size_t)nc) * 4; }

// One workgroup per sample.  Prologue: thread (h, d) walks the D vertices of hull h (all lanes of a wave read the same
// vertex when D is a multiple of 64); `>` keeps the first of equal values.  Test: lanes own candidates, the loops over
// hulls and directions are uniform over a wave, so dirs and support values are LDS broadcast reads; a hull is left at the
// first direction that says outside.  Compaction: one flag bit per (chunk, thread), ballot counts per (chunk, wave), an
// exclusive prefix by wave 0, then every survivor writes its index at its place (the pattern of cutmix_points_kernel).
__global__ __launch_bounds__(US_THREADS) void union_surface_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ keep, const float* __restrict__ dirs,
    const float* __restrict__ cand, const int32_t* __restrict__ cand_hull, int G, int D, int nc, int n_out, float margin,
    float* __restrict__ support, int32_t* __restrict__ outside, float* __restrict__ points, int32_t* __restrict__ src,
    int32_t* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) float us_lds[];
    float4* dir4 = reinterpret_cast<float4*>(us_lds);                  // [D]
    float* sup = us_lds + (size_t)D * 4;                               // [G,D]
    int* list = reinterpret_cast<int*>(sup + (size_t)G * D);           // [nc]
    __shared__ int woff[US_MAX_CHUNKS * US_WAVES + 1];
    __shared__ int kp[VPN_UNION_MAX_HULLS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* V = verts + (size_t)b * G * D * 3;
    const float* C = cand + (size_t)b * nc * 3;
    const int32_t* CH = cand_hull + (size_t)b * nc;

    for (int d = tid; d < D; d += US_THREADS) {
        const vpn::F3 v = vpn::ld3(dirs + (size_t)d * 3);
        dir4[d] = make_float4(v.x, v.y, v.z, 0.0f);
    }
    if (tid < G) kp[tid] = keep[(size_t)b * G + tid] != 0 ? 1 : 0;
    __syncthreads();
    for (int i = tid; i < G * D; i += US_THREADS) {
        const int h = i / D, d = i - h * D;
        const float4 dv = dir4[d];
        const float* hv = V + (size_t)h * D * 3;
        float best = am_dot(hv[0], hv[1], hv[2], dv.x, dv.y, dv.z);
        for (int j = 1; j < D; ++j) {
            const vpn::F3 p = vpn::ld3(hv + (size_t)j * 3);
            const float v = am_dot(p.x, p.y, p.z, dv.x, dv.y, dv.z);
            if (v > best) best = v;
        }
        sup[i] = best;
        support[(size_t)b * G * D + i] = best;
    }
    __syncthreads();

    const int nchunk = (nc + US_THREADS - 1) / US_THREADS, E = nchunk * US_WAVES;
    uint32_t mine = 0u;
    for (int k = 0; k < nchunk; ++k) {
        const int c = k * US_THREADS + tid;
        bool alive = false;
        if (c < nc) {
            const vpn::F3 p = vpn::ld3(C + (size_t)c * 3);
            const int own = CH[c];
            alive = (unsigned)own < (unsigned)G && kp[own] != 0;       // a candidate of a cut hull is rejected
            for (int h = 0; alive && h < G; ++h) {
                if (h == own || kp[h] == 0) continue;
                const float* sh = sup + (size_t)h * D;
                bool inside = true;
                for (int d = 0; d < D; ++d) {
                    const float4 dv = dir4[d];
                    if (am_dot(p.x, p.y, p.z, dv.x, dv.y, dv.z) > sh[d] - margin) { inside = false; break; }
                }
                if (inside) alive = false;
            }
            outside[(size_t)b * nc + c] = alive ? 1 : 0;
        }
        mine |= (alive ? 1u : 0u) << k;
        const u64 m = __ballot(alive);
        if (lane == 0) woff[k * US_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    if (wave == 0) {                                    // exclusive prefix over the (chunk, wave) counts
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
    for (int k = 0; k < nchunk; ++k) {
        const bool alive = ((mine >> k) & 1u) != 0u;
        const u64 m = __ballot(alive);
        if (alive) list[woff[k * US_WAVES + wave] + __popcll(m & ((1ull << lane) - 1ull))] = k * US_THREADS + tid;   // < cnt <= nc
    }
    __syncthreads();
    for (int i = tid; i < n_out; i += US_THREADS) {
        const int c = cnt > 0 ? list[i < cnt ? i : i % cnt] : i % nc;
        const vpn::F3 p = vpn::ld3(C + (size_t)c * 3);
        src[(size_t)b * n_out + i] = c;
        vpn::st3(points + ((size_t)b * n_out + i) * 3, p.x, p.y, p.z);
    }
    if (tid == 0) count[b] = cnt;
}

}  // namespace

extern "C" int vpn_hull_augment(const float* verts, const int32_t* group, const int32_t* coin, const float* u_num,
                                const float* scale, const int32_t* turn, const float* shift, const float* u_hull, int S, int G,
                                int D, int O, float* out, int32_t* keep, void* stream) {
    if (!verts || !group || !coin || !u_num || !scale || !turn || !shift || !u_hull || !out || !keep || S <= 0 || G <= 0 ||
        D <= 0 || O <= 0)
        return VPN_E_BADARG;
    if (G > VPN_UNION_MAX_HULLS || O > VPN_UNION_MAX_HULLS || D > VPN_UNION_MAX_DIRS || S > VPN_UNION_MAX_SAMPLES)
        return VPN_E_TOOBIG;                            // before any HIP call
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(hull_augment_kernel, dim3(O, S), dim3(HA_THREADS), 0, s, verts, group, coin, u_num, scale, turn, shift, u_hull,
               G, D, O, out, keep);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_union_surface(const float* verts, const int32_t* keep, const float* dirs, const float* cand,
                                 const int32_t* cand_hull, int S, int G, int D, int nc, int n_out, float margin,
                                 float* support, int32_t* outside, float* points, int32_t* src, int32_t* count,
                                 void* stream) {
    if (!verts || !keep || !dirs || !cand || !cand_hull || !support || !outside || !points || !src || !count || S <= 0 ||
        G <= 0 || D <= 0 || nc <= 0 || n_out <= 0 || !(margin == margin))
        return VPN_E_BADARG;
    if (G > VPN_UNION_MAX_HULLS || D > VPN_UNION_MAX_DIRS || S > VPN_UNION_MAX_SAMPLES || nc > VPN_UNION_MAX_CAND)
        return VPN_E_TOOBIG;                            // before any HIP call
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = us_lds_bytes(G, D, nc);
    if (lds > 49152) {      // dynamic LDS above the default limit is allowed for the kernel on the CURRENT device, per call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(union_surface_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)us_lds_bytes(VPN_UNION_MAX_HULLS, VPN_UNION_MAX_DIRS, VPN_UNION_MAX_CAND));
        if (e != hipSuccess) return (int)e;
    }
    VPN_LAUNCH(union_surface_kernel, dim3(S), dim3(US_THREADS), lds, s, verts, keep, dirs, cand, cand_hull, G, D, nc, n_out,
               margin, support, outside, points, src, count);
    VPN_LAUNCH_CHECK();
    return 0;
}
