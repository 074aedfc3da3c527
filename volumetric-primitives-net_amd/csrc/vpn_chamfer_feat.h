// vpn_chamfer_feat.h — the target-side features of the matrix-pipe Chamfer filter (fp32 planes + rows of 16-bit
// pieces + per-slice max norms) and the workgroup body that writes them.  Shared by chamfer.hip (chamfer_feat_kernel:
// both clouds of a Chamfer call) and sampler.hip (the forward launch of the training step writes the features of the
// cloud it has just sampled, and of the ground-truth cloud, so the feature kernel disappears from the step).
// Everything here is exact or covered by the filter's error bound whatever the translation unit's contraction mode.
#pragma once
#include "vpn_common.h"

namespace vpn {

constexpr int CM_ROWB = 48;              // bytes per bf16 row: K slots 0..15 for v_mfma_f32_32x32x16_bf16, 16..23 for v_mfma_f32_32x32x8_bf16
                                         // (21 used).  Also the LDS stride: 16 consecutive rows x 16 B hit 64 distinct banks (12 r mod 64)
// exact 3-way split of an fp32 into bf16 pieces (truncation): x == p0 + p1 + p2
__device__ inline void split3_bf16(float x, unsigned short p[3]) {
#pragma clang fp contract(off)
    const unsigned u0 = __float_as_uint(x);
    p[0] = (unsigned short)(u0 >> 16);
    const float r1 = x - __uint_as_float(u0 & 0xFFFF0000u);
    const unsigned u1 = __float_as_uint(r1);
    p[1] = (unsigned short)(u1 >> 16);
    const float r2 = r1 - __uint_as_float(u1 & 0xFFFF0000u);
    p[2] = (unsigned short)(__float_as_uint(r2) >> 16);
}

constexpr float CM_S16 = 2048.0f;                            // coordinate scale of the fp16 rows (2^11)
constexpr int CM_ROWB16 = 32;            // bytes per fp16 row in HBM (16 K slots); LDS stride stays 48 B (bank-conflict free)
// X = h[0] + h[1] + r with |r| <= 2^-22 |X| + 2^-25 (fp16 pieces, round to nearest)
__device__ inline void split2_f16(float X, _Float16 h[2]) {
    h[0] = (_Float16)X;
    h[1] = (_Float16)(X - (float)h[0]);
}

// one 32-byte row: K slots  x (b1 b1 b2), y (...), z (...), S^2 |p|^2 as p1 2^15 + p2 2^4 + p3, 4 zeros
struct Row16 { uint4 lo, hi; };
__device__ inline Row16 make_row16(float x, float y, float z, float n) {
#pragma clang fp contract(off)
    _Float16 hx[2], hy[2], hz[2], pn[3];
    split2_f16(CM_S16 * x, hx); split2_f16(CM_S16 * y, hy); split2_f16(CM_S16 * z, hz);
    if (n < 1.0e30f) {
        const float ns = (CM_S16 * CM_S16) * n;
        pn[0] = (_Float16)(ns * 3.0517578125e-05f);                     // 2^-15
        const float r1 = ns - (float)pn[0] * 32768.0f;
        pn[1] = (_Float16)(r1 * 0.0625f);                               // 2^-4
        pn[2] = (_Float16)(r1 - (float)pn[1] * 16.0f);
    } else {                                                            // padding sentinel: 65504 * 2^15 / S^2 = 512 > any t in range
        pn[0] = (_Float16)65504.0f; pn[1] = (_Float16)0.0f; pn[2] = (_Float16)0.0f;
    }
    auto bits = [](_Float16 v) { return (unsigned)__builtin_bit_cast(unsigned short, v); };
    auto pk = [&](_Float16 lo, _Float16 hi) { return bits(lo) | (bits(hi) << 16); };
    const _Float16 zero = (_Float16)0.0f;
    return Row16{make_uint4(pk(hx[0], hx[0]), pk(hx[1], hy[0]), pk(hy[0], hy[1]), pk(hz[0], hz[0])),
                 make_uint4(pk(hz[1], pn[0]), pk(pn[1], pn[2]), pk(zero, zero), pk(zero, zero))};
}
// the row of a padding target (x = y = z = 0, the never-winning sentinel norm): what feat_point writes for rows j >= N
__device__ inline Row16 sentinel_row16() { return make_row16(0.0f, 0.0f, 0.0f, 3.0e38f); }
__device__ inline void write_row16(unsigned short* H, size_t row, float x, float y, float z, float n) {
    const Row16 r = make_row16(x, y, z, n);
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(H) + row * CM_ROWB16);
    dst[0] = r.lo; dst[1] = r.hi;
}

// feature planes F[b][4][Np] = (x, y, z, |p|^2) (padded with a never-winning sentinel) and
// H[b][Np][24] bf16 rows (48 B) for the bf16 filter: per coordinate the target pieces (b1 b1 b2 b1 b3 b2) that pair
// with the query pieces (a1 a2 a1 a3 a1 a2), then the three pieces of |p|^2 (paired with 1.0), then zeros.
// nmax[b][CFEAT_SLOTS]: max |p|^2 of each workgroup's slice (the filter takes the max of the slots: no atomics,
// no zero-initialised output, no workgroup that scans the whole cloud).
// one 48-byte row of bf16 pieces: K slots  x (b1 b1 b2 b1 b3 b2), y (...), z (...), |p|^2 (3 pieces), 3 zeros
__device__ inline void write_row(unsigned short* H, size_t row, float x, float y, float z, float n) {
#pragma clang fp contract(off)
    unsigned short px[3], py[3], pz[3], pn[3];
    split3_bf16(x, px); split3_bf16(y, py); split3_bf16(z, pz); split3_bf16(n, pn);
    auto pk = [](unsigned short lo, unsigned short hi) { return (unsigned)lo | ((unsigned)hi << 16); };
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(H) + row * CM_ROWB);
    dst[0] = make_uint4(pk(px[0], px[0]), pk(px[1], px[0]), pk(px[2], px[1]), pk(py[0], py[0]));
    dst[1] = make_uint4(pk(py[1], py[0]), pk(py[2], py[1]), pk(pz[0], pz[0]), pk(pz[1], pz[0]));
    dst[2] = make_uint4(pk(pz[2], pz[1]), pk(pn[0], pn[1]), pk(pn[2], 0), 0u);
}


constexpr int CFEAT_THREADS = 256;
#ifndef CFEAT_WGPTS
#define CFEAT_WGPTS 256             // points per feature workgroup (1024: r1; 256: 4x the workgroups, the kernel is latency-bound)
#endif
constexpr int CFEAT_SLOTS = 64;                    // slices (workgroups) per cloud and sample, at most: one lane each in the scan's epilogue
constexpr int CFEAT_PTS = 4;                       // points per lane in flight

struct FeatJob {          // one cloud: slices [0, ysplit) of a sample's workgroups belong to it
    const float* pts; int N, Np, ysplit;
    float* F; unsigned int* nmax; unsigned short* H;
    int rows16;           // rows as 32-byte fp16 pieces (PREC 2) instead of 48-byte bf16 pieces (PREC 1)
    float* tboxes;        // fp16 filter, cloud in the TARGET role of the skipping scan: a box per 256-row tile (or null)
    int32_t* perm;        // fp16 filter, cloud in the QUERY role of that scan: its points in Morton-cell order (or null)
};

// workgroup id -> (sample, slice): sample b runs on XCD b / (B/8), where the filter kernel reads what is written
__device__ inline void feat_decode(int id, int B, int& b, int& sy) {
    const int per = B >> 3;
    if ((B & 7) == 0) { const int xcd = id & 7, r = id >> 3; b = xcd * per + r % per; sy = r / per; }
    else { b = id % B; sy = id / B; }
}

__device__ inline float feat_wave_max(float v) {      // values >= 0
#define VPN_FDPP(v, ctrl, rmask) \
    __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), ctrl, rmask, 0xf, false))
    v = fmaxf(v, VPN_FDPP(v, 0x111, 0xf)); v = fmaxf(v, VPN_FDPP(v, 0x112, 0xf));
    v = fmaxf(v, VPN_FDPP(v, 0x114, 0xf)); v = fmaxf(v, VPN_FDPP(v, 0x118, 0xf));
    v = fmaxf(v, VPN_FDPP(v, 0x142, 0xa)); v = fmaxf(v, VPN_FDPP(v, 0x143, 0xc));
#undef VPN_FDPP
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// planes and row of ONE point (j < Np; a padding point j >= N gets the never-winning sentinel); returns |p|^2 (0 for padding)
__device__ inline float feat_point(const FeatJob& J, int b, int j, float x, float y, float z) {
#pragma clang fp contract(off)
    float* f = J.F + (size_t)b * 4 * J.Np;
    float n = 3.0e38f, nv = 0.0f;
    if (j < J.N) { n = x * x + y * y + z * z; nv = n; } else { x = 0.f; y = 0.f; z = 0.f; }
    f[j] = x; f[J.Np + j] = y; f[2 * J.Np + j] = z; f[3 * J.Np + j] = n;
    if (J.H) {
        if (J.rows16) write_row16(J.H, (size_t)b * J.Np + j, x, y, z, n);
        else write_row(J.H, (size_t)b * J.Np + j, x, y, z, n);
    }
    return nv;
}

// per-workgroup bookkeeping of a slice: the max norm of the slice into its slot; slice 0 also zeroes the slots no
// slice owns.  `red`: CFEAT_THREADS / 64 floats of LDS.  Contains a barrier.
__device__ inline void feat_finish_slice(const FeatJob& J, int b, int by, float nv, float* red) {
    if (by == 0 && (int)threadIdx.x >= J.ysplit && threadIdx.x < CFEAT_SLOTS) J.nmax[b * CFEAT_SLOTS + threadIdx.x] = 0u;
    nv = feat_wave_max(nv);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nv;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = red[0];
        for (int w = 1; w < CFEAT_THREADS / 64; ++w) m = fmaxf(m, red[w]);
        J.nmax[b * CFEAT_SLOTS + by] = __float_as_uint(m);
    }
}

template <bool MAX>
__device__ inline float feat_wave_minmax(float v) {   // any finite or infinite values; the result is wave-uniform
#define VPN_FDPP(v, ctrl, rmask) \
    __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), ctrl, rmask, 0xf, false))
#define VPN_FOP(a, b) (MAX ? fmaxf(a, b) : fminf(a, b))
    v = VPN_FOP(v, VPN_FDPP(v, 0x111, 0xf)); v = VPN_FOP(v, VPN_FDPP(v, 0x112, 0xf));
    v = VPN_FOP(v, VPN_FDPP(v, 0x114, 0xf)); v = VPN_FOP(v, VPN_FDPP(v, 0x118, 0xf));
    v = VPN_FOP(v, VPN_FDPP(v, 0x142, 0xa)); v = VPN_FOP(v, VPN_FDPP(v, 0x143, 0xc));
#undef VPN_FOP
#undef VPN_FDPP
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- Tile skipping of the fp16 scan (chamfer.hip, direction 2 of a Chamfer call).  The scan's LDS tiles are 256
// consecutive target rows; a wave skips a tile when every one of its 32 queries provably has a nearer target already
// (DESIGN 4.1).  That needs (a) a box per target tile and (b) waves of queries that lie close together, so the query
// cloud is visited in Morton-cell order (a permutation; the features themselves stay in the original order).
constexpr int CFEAT_TILE = 256;          // rows per tile box (= CM_TILE16 of the scan)
constexpr int CFEAT_BOXF = 8;            // floats per box: lo xyz, hi xyz, 2 unused
// the skipping scan is used when direction 2 has at least this many targets (the sampled cloud): measured, at 2048 targets
// (8 tiles, the C5 step's clouds) the ordering workgroups cost more than the skipped tiles save
constexpr int CSKIP_MIN_TARGETS = 4096;
constexpr int CORD_MAX = 2048;           // largest cloud one workgroup orders (8 cells per lane in registers); larger
                                         // clouds keep their natural order
// Candidate form of the scan (chamfer.hip): a workgroup whose 256 queries lie close together scans only the
// targets inside a ball around them.  Taken by a direction without tile boxes from CSKIP_MIN_TARGETS queries on.
constexpr int CCAND_CAP = 512;           // candidates per workgroup at most (= the two 256-row LDS tiles as one buffer)
constexpr int CCAND_MAX_TARGETS = 65535; // candidate indices are kept as 16-bit numbers
constexpr int CCAND_CELL = 16;           // compact positions per tracked cell of the candidate loop (a quarter of a pair of blocks)

// box entry of tile t of sample b of a cloud with Np padded rows (the workspace carves Np / 32 entries per sample)
__device__ inline float* feat_tile_box(float* boxes, int Np, int b, int t) {
    return boxes + ((size_t)b * (Np >> 5) + t) * CFEAT_BOXF;
}

// The boxes of the tiles that meet the rows [rlo, rhi) of sample b, whose planes this workgroup has written (the caller
// orders those writes before this call with a fence and a barrier).  A tile that lies entirely inside [rlo, rhi) gets
// the exact box of its points (padding rows excluded; a tile of padding only gets the empty box +inf / -inf); a tile
// the workgroup shares with another gets the box of all space (never skipped) -- every writer of it writes those same
// bits.  One wave per tile.
__device__ inline void feat_tile_boxes(const FeatJob& J, int b, int rlo, int rhi) {
    if (!J.tboxes || rlo >= rhi) return;
    const float* f = J.F + (size_t)b * 4 * J.Np;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inf = __builtin_inff();
    for (int t = rlo / CFEAT_TILE + wave; t * CFEAT_TILE < rhi; t += CFEAT_THREADS / 64) {
        const int r0 = t * CFEAT_TILE, r1 = min(r0 + CFEAT_TILE, J.Np);
        float lo[3] = {-inf, -inf, -inf}, hi[3] = {inf, inf, inf};
        if (r0 >= rlo && r1 <= rhi) {                               // uniform per wave
            lo[0] = lo[1] = lo[2] = inf; hi[0] = hi[1] = hi[2] = -inf;
            const int rn = min(r1, J.N);
            for (int r = r0 + lane; r < rn; r += 64) {
                const float x = f[r], y = f[J.Np + r], z = f[2 * J.Np + r];
                lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
                lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
                lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = feat_wave_minmax<false>(lo[a]); hi[a] = feat_wave_minmax<true>(hi[a]); }
        }
        if (lane == 0) {
            float4* o = reinterpret_cast<float4*>(feat_tile_box(J.tboxes, J.Np, b, t));
            o[0] = make_float4(lo[0], lo[1], lo[2], hi[0]);
            o[1] = make_float4(hi[1], hi[2], 0.f, 0.f);
        }
    }
}

// The query order of sample b of the cloud J.pts: J.perm[b][s] = the point visited s-th.  A stable counting sort by the
// 4 x 4 x 4 Morton cell of the sample's bounding box (deterministic: the order inside a cell is the original one), by one
// workgroup of CFEAT_THREADS lanes.  Lane l of wave w holds the cells of the points w * 64 + l + 256 j (j < CORD_PER),
// i.e. lane l of every chunk c = w + 4 j of 64 consecutive points: the rank of a point among the chunk's points of its
// cell comes from six ballots, a table [chunk][cell] of counts in LDS turns into the output positions.  Clouds above
// CORD_MAX points keep their natural order.  Rows past N are not written (the scan never uses them).
__device__ inline void feat_order_wg(const FeatJob& J, int b) {
    constexpr int CORD_PER = CORD_MAX / CFEAT_THREADS;
    __shared__ unsigned short cnt[CORD_MAX / 64][64];
    __shared__ float bred[6][CFEAT_THREADS / 64];
    __shared__ int cbase[64];
    const int N = J.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* p = J.pts + (size_t)b * N * 3;
    int32_t* po = J.perm + (size_t)b * J.Np;
    if (N > CORD_MAX) {
        for (int i = tid; i < N; i += CFEAT_THREADS) po[i] = i;
        return;
    }
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll 2
    for (int j = 0; j < CORD_PER; ++j) {                            // (unrolled little: the sampler's register budget)
        const F3 v = ld3(p + min(tid + j * CFEAT_THREADS, N - 1) * 3);     // a repeated point changes no box
        lo[0] = fminf(lo[0], v.x); hi[0] = fmaxf(hi[0], v.x);
        lo[1] = fminf(lo[1], v.y); hi[1] = fmaxf(hi[1], v.y);
        lo[2] = fminf(lo[2], v.z); hi[2] = fmaxf(hi[2], v.z);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = feat_wave_minmax<false>(lo[a]), h = feat_wave_minmax<true>(hi[a]);
        if (lane == 0) { bred[a][wave] = l; bred[3 + a][wave] = h; }
    }
    const int nch = (N + 63) >> 6;
    for (int e = tid; e < nch * 64; e += CFEAT_THREADS) cnt[e >> 6][e & 63] = 0;
    __syncthreads();
    float o3[3], sc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = bred[a][0], h = bred[3 + a][0];
        for (int w = 1; w < CFEAT_THREADS / 64; ++w) { l = fminf(l, bred[a][w]); h = fmaxf(h, bred[3 + a][w]); }
        o3[a] = l;
        sc[a] = h > l ? 4.0f / (h - l) : 0.0f;                      // non-finite boxes give cell 0 (the order is only speed)
    }
    static_assert(CORD_PER * 6 <= 64, "the cells of a lane's points are packed into 64 bits");
    unsigned long long keys = 0;                                    // cell of point j in bits [6 j, 6 j + 6)
#pragma unroll 2
    for (int j = 0; j < CORD_PER; ++j) {                            // the points again (L2 hits)
        const F3 v = ld3(p + min(tid + j * CFEAT_THREADS, N - 1) * 3);
        const float c[3] = {v.x, v.y, v.z};
        unsigned k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned ca = (unsigned)(int)fminf(fmaxf((c[a] - o3[a]) * sc[a], 0.0f), 3.0f);   // NaN -> 0
            k |= ((ca & 1u) << a) | ((ca >> 1) << (a + 3));
        }
        keys |= (unsigned long long)k << (6 * j);
    }
    // rank of lane among the chunk's lanes of the same cell, and how many there are
    auto rank_of = [&](unsigned k, bool ok, int& rank, int& count) {
        unsigned long long eq = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 6; ++bit) {
            const bool s = (k >> bit) & 1u;
            const unsigned long long m = __ballot(s);
            eq &= s ? m : ~m;
        }
        rank = __popcll(eq & ((1ull << lane) - 1ull));
        count = __popcll(eq);
    };
#pragma unroll 2
    for (int j = 0; j < CORD_PER; ++j) {                            // pass 1: counts per (chunk, cell)
        const int c = wave + j * (CFEAT_THREADS / 64);
        if (c >= nch) break;                                        // uniform per wave
        const bool ok = tid + j * CFEAT_THREADS < N;
        const unsigned k = (unsigned)(keys >> (6 * j)) & 63u;
        int rank, count;
        rank_of(k, ok, rank, count);
        if (ok && rank == 0) cnt[c][k] = (unsigned short)count;
    }
    __syncthreads();
    if (tid < 64) {                                                 // per cell: exclusive prefix over the chunks
        int s = 0;
#pragma unroll 8
        for (int c = 0; c < nch; ++c) { const int t = cnt[c][tid]; cnt[c][tid] = (unsigned short)s; s += t; }
        int inc = s;                                                // ... and over the cells
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t2 = __shfl_up(inc, o, 64); if (lane >= o) inc += t2; }
        cbase[tid] = inc - s;
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < CORD_PER; ++j) {                            // pass 2: positions
        const int c = wave + j * (CFEAT_THREADS / 64);
        if (c >= nch) break;
        const int i = tid + j * CFEAT_THREADS;
        const bool ok = i < N;
        const unsigned k = (unsigned)(keys >> (6 * j)) & 63u;
        int rank, count;
        rank_of(k, ok, rank, count);
        if (ok) po[cbase[k] + cnt[c][k] + rank] = i;
    }
}

// slice `by` of sample b of the cloud J.pts (AoS xyz): one workgroup of CFEAT_THREADS lanes
__device__ inline void feat_slice(const FeatJob& J, int b, int by, float* red) {
    const float* pb = J.pts + (size_t)b * J.N * 3;
    float nv = 0.f;
    const int per = ((J.Np + J.ysplit - 1) / J.ysplit + 63) & ~63;
    const int jlo = by * per, jhi = min(J.Np, jlo + per);
    for (int j0p = jlo + threadIdx.x; j0p < jhi; j0p += CFEAT_PTS * CFEAT_THREADS) {
        float xs[CFEAT_PTS], ys[CFEAT_PTS], zs[CFEAT_PTS];
#pragma unroll
        for (int u = 0; u < CFEAT_PTS; ++u) {
            const int j = min(j0p + u * CFEAT_THREADS, J.N - 1);
            const F3 v3 = ld3(pb + j * 3);
            xs[u] = v3.x; ys[u] = v3.y; zs[u] = v3.z;
        }
#pragma unroll
        for (int u = 0; u < CFEAT_PTS; ++u) {
            const int j = j0p + u * CFEAT_THREADS;
            if (j >= jhi) break;
            nv = fmaxf(nv, feat_point(J, b, j, xs[u], ys[u], zs[u]));
        }
    }
    if (J.tboxes) __threadfence_block();                            // the planes, for the tile boxes behind the barrier
    feat_finish_slice(J, b, by, nv, red);
    feat_tile_boxes(J, b, jlo, jhi);
}

// The same slice by the lanes [first, CFEAT_THREADS) of a workgroup and WITHOUT its barrier: the caller has one coming
// anyway (the sampler's pose barrier: the slice's loads then overlap the pose lane's chain instead of forming a phase of
// their own behind the sampling).  The waves' max norms go to red[wave]; after the caller's barrier ONE lane calls
// feat_slice_publish.  `first` is a multiple of 64.
__device__ inline void feat_slice_early(const FeatJob& J, int b, int by, int first, float* red) {
    if (by == 0 && (int)threadIdx.x >= J.ysplit && threadIdx.x < CFEAT_SLOTS) J.nmax[b * CFEAT_SLOTS + threadIdx.x] = 0u;
    if ((int)threadIdx.x < first) return;
    const float* pb = J.pts + (size_t)b * J.N * 3;
    float nv = 0.f;
    const int per = ((J.Np + J.ysplit - 1) / J.ysplit + 63) & ~63;
    const int jlo = by * per, jhi = min(J.Np, jlo + per), lanes = CFEAT_THREADS - first;
    for (int j = jlo + (int)threadIdx.x - first; j < jhi; j += lanes) {
        const F3 v3 = ld3(pb + min(j, J.N - 1) * 3);
        nv = fmaxf(nv, feat_point(J, b, j, v3.x, v3.y, v3.z));
    }
    nv = feat_wave_max(nv);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nv;
}
__device__ inline void feat_slice_publish(const FeatJob& J, int b, int by, int first, const float* red) {
    float m = red[first >> 6];
    for (int w = (first >> 6) + 1; w < CFEAT_THREADS / 64; ++w) m = fmaxf(m, red[w]);
    J.nmax[b * CFEAT_SLOTS + by] = __float_as_uint(m);
}

// host side (chamfer.hip): the two feature jobs of the fp16 filter inside a caller-provided Chamfer workspace, in the
// layout vpn_chamfer_fwd_ws(mode 7) expects.  p1 [B,N,3] is the cloud the caller is about to write (pts may be its
// address or null), p2 [B,M,3] the other one.  Returns 0, or VPN_E_BADARG if the workspace is short / misaligned or the
// automatic mode would not take the fp16 filter for these sizes.
int chamfer_feat_jobs(void* workspace, size_t workspace_bytes, int B, int N, int M, const float* p1, const float* p2,
                      FeatJob* job1, FeatJob* job2);
// the per-workgroup sums of the minima the fp16 scan leaves in that workspace: sums1 [B][*g1] (dist1), sums2 [B][*g2] (dist2)
int chamfer_wgsums(const void* workspace, size_t workspace_bytes, int B, int N, int M, const float** sums1, int* g1,
                   const float** sums2, int* g2);

}  // namespace vpn
