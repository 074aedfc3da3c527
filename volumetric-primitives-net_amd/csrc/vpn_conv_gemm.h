// vpn_conv_gemm.h — the implicit GEMM D[m][n] = sum_k A[m][k] B[k][n] on the f32-input MFMA that csrc/trunkconv.hip,
// csrc/trunkstride.hip and csrc/trunkfold.hip share: everything that does not depend on how an operand element is found.
//   * cg_tile: a workgroup of 256 (4 waves, 2 x 2) owns a 64 x 64 tile of D, every wave a 32 x 32 quarter in 16 accumulator
//     registers of v_mfma_f32_32x32x2_f32; K is walked in chunks of 16 through LDS ([k][m] and [k][n], so a wave reads its
//     operands along consecutive lanes), the next chunk's global loads are issued before the current chunk's MFMAs.  Where
//     an element of A or B lives, and whether it exists, is the staging map's business (the template parameter);
//   * cg_plan: a product with fewer than VPN_CONV_SPLIT_TARGET tiles splits K over gridDim.z slices of whole chunks
//     (balanced: slice z owns the chunks [z n / S, (z + 1) n / S)); a slice writes its partial tile to the caller's
//     workspace [S][D] and cg_merge adds the S partials of every element in the order 0 .. S - 1;
//   * one summation order: inside a slice the k-ordered fmaf chain of the MFMA, then the slices in order.  No atomics, no
//     grid barrier, nothing allocated, no host synchronisation: bit-equal from run to run and capturable;
//   * the merge uses 16-byte accesses when the element count is a multiple of 4 and the output 16-byte aligned, element
//     accesses otherwise.
// A staging map is constructed from (args, m0, n0, tid), names B's LDS layout (B_K_FASTEST) and has load(args, chunk, stage):
// the work-item's CG_PER elements of each operand of that chunk in cg_store's order, 0.0f for one that does not exist (no
// address formed).  A kernel's args struct has a, b, out, M, N, K, chunks, S and total as cg_fill sets them, and PHW, the
// pixels per image of the image the pixel index runs over: n of a PIXELS product, where cg_tile's epilogue divides by it to
// place the NCHW result; k of a weight gradient, where only the staging map reads it (the epilogue does not).
#pragma once
#include "vpn_common.h"

namespace vpn {

constexpr int CG_T = VPN_CONV_TILE;          // rows and columns of D a workgroup owns
constexpr int CG_K = VPN_CONV_TILE_K;        // reduction elements per LDS chunk
constexpr int CG_BLOCK = 256;
constexpr int CG_LD = CG_T + 32;             // LDS row pitch: the two k rows a wave reads per MFMA land on disjoint banks
constexpr int CG_PER = CG_T * CG_K / CG_BLOCK;     // elements of each operand a work-item stages per chunk
static_assert(CG_T == 64 && CG_K == 16 && CG_PER == 4, "the staging maps are written for 64 x 64 x 16 and 256 work-items");

#ifndef VPN_HOST_SHIM
typedef float f32x16 __attribute__((ext_vector_type(16)));
#endif

// what a work-item holds between the global loads of a chunk and its LDS stores
struct CgStage { float a[CG_PER], b[CG_PER]; };

// A work-item's CG_PER elements of each operand into LDS.  A is staged k fastest: element j is (k, m) = (tid & 15,
// (tid >> 4) + 16 j) of the chunk.  B likewise when K_FASTEST, else column fastest: (k, n) = ((tid >> 6) + 4 j, tid & 63).
template <bool B_K_FASTEST>
__device__ __forceinline__ void cg_store(const CgStage& st, float (*As)[CG_LD], float (*Bs)[CG_LD], int tid) {
#pragma unroll
    for (int j = 0; j < CG_PER; ++j) {
        As[tid & 15][(tid >> 4) + 16 * j] = st.a[j];
        if (B_K_FASTEST) Bs[tid & 15][(tid >> 4) + 16 * j] = st.b[j];
        else Bs[(tid >> 6) + 4 * j][tid & 63] = st.b[j];
    }
}

// What cg_tile does with a finished element: `v` belongs at out[idx], row m of D.  The default stores it as it is; a kernel
// with more to do at the store (csrc/trunkfold.hip: bias, residual, ReLU) names its own.
struct CgPlainStore {
    template <class Args>
    __device__ static __forceinline__ void store(const Args&, float* out, size_t idx, unsigned, float v) { out[idx] = v; }
};

// One tile of one slice; grid (tiles of N, tiles of M, S).  PIXELS: column n of D is pixel n % PHW of image n / PHW of an
// NCHW result with M channels (forward, data gradient); otherwise D is stored row-major (weight gradient).  Forced inline
// with the args by value, as the kernel holds them: behind a reference the compiler schedules the loop differently.
template <class Map, bool PIXELS, class Epilogue = CgPlainStore, class Args>
__device__ __forceinline__ void cg_tile(const Args g) {
    __shared__ float As[CG_K][CG_LD];
    __shared__ float Bs[CG_K][CG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n0 = blockIdx.x * CG_T, m0 = blockIdx.y * CG_T, z = blockIdx.z;
    if (m0 >= g.M || n0 >= g.N || z >= (unsigned)g.S) return;          // the host never asks
    const unsigned c0 = (unsigned)((unsigned long long)z * g.chunks / g.S);
    const unsigned c1 = (unsigned)((unsigned long long)(z + 1) * g.chunks / g.S);
    Map map(g, m0, n0, tid);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, col = lane & 31, half = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    CgStage st;
    if (c0 < c1) map.load(g, c0, st);
    for (unsigned c = c0; c < c1; ++c) {
        __syncthreads();                                     // the previous chunk has been read by every wave
        cg_store<Map::B_K_FASTEST>(st, As, Bs, tid);
        __syncthreads();
        if (c + 1 < c1) map.load(g, c + 1, st);
#pragma unroll
        for (int t = 0; t < CG_K / 2; ++t)                   // lane: A[row col][k half], B[k half][column col]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * t + half][wm + col], Bs[2 * t + half][wn + col], acc, 0, 0, 0);
    }
    // D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const unsigned n = n0 + wn + col;
    if (n >= g.N) return;
    float* out = g.out + (size_t)z * g.total;
    size_t base, pitch;
    if (PIXELS) {
        const unsigned b = n / g.PHW;
        base = (size_t)b * g.M * g.PHW + (n - b * g.PHW); pitch = g.PHW;
    } else {
        base = n; pitch = g.N;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < g.M) Epilogue::store(g, out, base + (size_t)m * pitch, m, acc[r]);
    }
}

__device__ inline void cg_add(float& r, float q) { r += q; }
__device__ inline void cg_add(float4& r, const float4& q) { r.x += q.x; r.y += q.y; r.z += q.z; r.w += q.w; }

// out[i] = ws[0][i] + ws[1][i] + ... + ws[S - 1][i], in that order, for `units` elements of T (float, or float4 for 16-byte
// accesses); `pitch`: the elements of T in a partial
template <class T>
__global__ __launch_bounds__(CG_BLOCK) void cg_merge_kernel(const T* ws, T* out, long long units, long long pitch, int S) {
    const long long u = (long long)blockIdx.x * CG_BLOCK + threadIdx.x;
    if (u >= units) return;
    T r = ws[u];
    for (int s = 1; s < S; ++s) cg_add(r, ws[(size_t)s * pitch + u]);
    out[u] = r;
}

// ---- the host rule: tiles, chunks and slices of one product
struct CgPlan { unsigned M, N, K; int chunks, S; unsigned mt, nt; long long total; };

// D[M][N] over K with `total` result elements
static int cg_plan(unsigned M, unsigned N, unsigned K, long long total, CgPlan* p) {
    p->M = M; p->N = N; p->K = K; p->total = total;
    p->mt = (M + CG_T - 1) / CG_T;
    p->nt = (unsigned)(((unsigned long long)N + CG_T - 1) / CG_T);
    if (p->mt > 65535u) return VPN_E_TOOBIG;                         // gridDim.y
    p->chunks = (int)(((unsigned long long)K + CG_K - 1) / CG_K);
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

static size_t cg_ws_bytes(const CgPlan& p) { return p.S > 1 ? (size_t)p.S * (size_t)p.total * sizeof(float) : 0; }

// the product needs a workspace and the caller's is missing, too small or not 16-byte aligned
static bool cg_ws_bad(const CgPlan& p, const void* ws, size_t bytes) {
    const size_t need = cg_ws_bytes(p);
    return need && (!ws || bytes < need || ((uintptr_t)ws & 15));
}

// the fields of a kernel's args that the plan decides; a split product writes its partials to the workspace
template <class Args>
static void cg_fill(Args& g, const CgPlan& p, const float* a, const float* b, float* out, void* ws) {
    g.a = a; g.b = b; g.out = p.S > 1 ? (float*)ws : out;
    g.M = p.M; g.N = p.N; g.K = p.K; g.chunks = p.chunks; g.S = p.S; g.total = p.total;
}

// after the GEMM launch of a split product: the partials of the workspace into `out`.  A template (Plan is CgPlan) so that
// only a file that calls it instantiates cg_merge_kernel: csrc/trunkfold.hip merges with an epilogue of its own
template <class Plan>
static int cg_merge(const Plan& p, const void* ws, float* out, hipStream_t st) {
    if (p.S == 1) return 0;
    const bool vec = p.total % 4 == 0 && ((uintptr_t)out & 15) == 0;          // the workspace is 16-byte aligned (checked)
    const long long units = vec ? p.total / 4 : p.total;
    const dim3 mg((unsigned)((units + CG_BLOCK - 1) / CG_BLOCK));
    if (vec) VPN_LAUNCH_AS("cg_merge_kernel", (cg_merge_kernel<float4>), mg, dim3(CG_BLOCK), 0, st, (const float4*)ws, (float4*)out, units, units, p.S);
    else VPN_LAUNCH_AS("cg_merge_kernel", (cg_merge_kernel<float>), mg, dim3(CG_BLOCK), 0, st, (const float*)ws, out, units, units, p.S);
    VPN_LAUNCH_CHECK();
    return 0;
}

}  // namespace vpn
