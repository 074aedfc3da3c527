// gcn.hip — the refinement stage of the reference (modules/network/gcn.py, GCNModel) around its dense GEMMs.
//
//   gcn_aggregate_kernel   out[b,i,:] = sum_j A[i,j] x[b,j,:] + bias (+ ReLU): the propagation of PyG's GCNConv over the
//                          CSR form of A = D^-1/2 (A_mesh + I) D^-1/2 (built on the host, ops.gcn_graph).  A is symmetric,
//                          so the backward is the same gather on the ReLU-masked gradient.
//   gcn_colsum_*           fixed-order column sums (dbias, the gradient of the global features)
//   gcn_bounds_kernel      get_bound_of_images (gcn.py:90-133) on the device, one workgroup per image
//   gcn_extent_kernel      per-sample min / max of z and y (and their first arg-extremes), then the pooling grid of
//                          every vertex (gcn.py:141-153)
//   gcn_input_kernel       conv1's input rows [encoding (0 | 3 | 39) | pooled (sum C_l) | global (G)] (gcn.py:36-42,
//                          :73-82, :155-163): bilinear, align_corners = True, zero padding, as grid_sample
//   gcn_pool_sort_kernel   backward: per (sample, level) the vertices sorted by bilinear cell (stable), so that
//   gcn_pool_bwd_kernel    every feature-map pixel sums the vertices that touch it in a fixed order: no atomics
//   gcn_vertex_bwd_kernel  backward to the vertices through the encoding and the grid
//   gcn_extent_bwd_kernel  ... and through the min / max (to the arg-extreme vertex, as torch.max(0) backward)
//   gcn_factored_*         conv1's product x Theta without the input row: every vertex gathers from the maps
//                          projected by Theta's row blocks; backward to Theta's encoding rows and to the vertices, the
//                          projected maps' gradient by gcn_pool_sort_kernel / gcn_pool_bwd_kernel with Cout channels a level
//
// Feature maps are read NHWC (one transpose per call, gcn_nhwc_kernel): a vertex's channels are then contiguous and a
// wave's 64 lanes read two 128-byte lines per corner instead of 64.
#include <climits>

#include "vpn_common.h"

namespace vpn {

constexpr int GCN_MAX_LEVELS = 4;
constexpr int GCN_SORT_MAX_N = 8192;     // vertices per sample the backward sorts in LDS (32-bit keys, 13 index bits)
constexpr int GCN_SORT_VBITS = 13;
constexpr int GCN_COLSUM_ROWS = 64;      // rows per partial column sum

struct GcnLevels {
    const float* map[GCN_MAX_LEVELS];    // NCHW, the caller's tensors
    float* dmap[GCN_MAX_LEVELS];         // NCHW gradients (backward)
    int C[GCN_MAX_LEVELS], H[GCN_MAX_LEVELS], W[GCN_MAX_LEVELS];
    int coff[GCN_MAX_LEVELS];            // first channel of level l in the pooled block
    int moff[GCN_MAX_LEVELS];            // first float of level l in one sample's NHWC copy
    int cstart[GCN_MAX_LEVELS];          // first cell-start slot of level l in one sample's sort workspace
    int L, ctot_pool, msize;             // levels, sum C_l, sum C_l H_l W_l
    int cs_size;                         // sum over levels of (H_l + 1)(W_l + 1) + 2
};

// ---------------------------------------------------------------------------------------------------------------------
// aggregation: one thread per (row, V channels); V = 4 reads and writes dwordx4 (C % 4 == 0)
template <int V>
__global__ __launch_bounds__(256) void gcn_aggregate_kernel(const float* __restrict__ x, const int* __restrict__ row_ptr,
                                                            const int* __restrict__ col, const float* __restrict__ w,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ mask, int N, int C, int relu,
                                                            long long total, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int cv = C / V;
    const long long row = t / cv;                  // b * N + i
    const int c = (int)(t - row * cv) * V;
    const int i = (int)(row % N);
    const long long base = row - i;                // b * N
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.0f;
    const int e1 = row_ptr[i + 1];
    for (int e = row_ptr[i]; e < e1; ++e) {
        const long long src = (base + col[e]) * C + c;
        const float a = w[e];
        float v[V];
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + src);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            if (mask) {
                const float4 m = *reinterpret_cast<const float4*>(mask + src);
                v[0] = m.x > 0.0f ? v[0] : 0.0f; v[1] = m.y > 0.0f ? v[1] : 0.0f;
                v[2] = m.z > 0.0f ? v[2] : 0.0f; v[3] = m.w > 0.0f ? v[3] : 0.0f;
            }
        } else {
            v[0] = x[src];
            if (mask && !(mask[src] > 0.0f)) v[0] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(a, v[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (bias) acc[k] += bias[c + k];
        if (relu) acc[k] = fmaxf(acc[k], 0.0f);
    }
    float* o = out + row * C + c;
    if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else o[0] = acc[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// column sums out[s, c] = sum_r in[(s R + r) ld + off + c] (* [mask > 0]) in a fixed order: partial sums over 64-row chunks,
// then the chunks in order
__global__ __launch_bounds__(256) void gcn_colsum_partial_kernel(const float* __restrict__ in,
                                                                 const float* __restrict__ mask, int R, int ld, int off,
                                                                 int C, int P, float* __restrict__ ws) {
    const int c = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y, s = blockIdx.z;
    if (c >= C) return;
    const int r0 = p * GCN_COLSUM_ROWS, r1 = min(R, r0 + GCN_COLSUM_ROWS);
    float acc = 0.0f;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) {
        const long long k = ((long long)s * R + r) * ld + off + c;
        const float v = in[k];
        acc += (mask && !(mask[k] > 0.0f)) ? 0.0f : v;
    }
    ws[((long long)s * P + p) * C + c] = acc;
}

__global__ __launch_bounds__(256) void gcn_colsum_final_kernel(const float* __restrict__ ws, int C, int P,
                                                               float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (c >= C) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int p = 0; p < P; ++p) acc += ws[((long long)s * P + p) * C + c];
    out[(long long)s * C + c] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// get_bound_of_images, read literally: mask = sum_c img (channels in order) > 0.03; b0 = min{i >= 1 : column i occupied}
// else 0 (0 means "unset" in the reference's loop, so column 0 never sets it), b1 = max{j : column j occupied} else w;
// rows alike; then b / w * 2 - 1 (b / h * 2 - 1) in fp32.  min / max are order-free: the result is exact.
__global__ __launch_bounds__(1024) void gcn_bounds_kernel(const float* __restrict__ img, int C, int H, int W,
                                                         float* __restrict__ bounds) {
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    const long long hw = (long long)H * W;
    const float* im = img + (long long)b * C * hw;
    int xlo = INT_MAX, xhi = -1, ylo = INT_MAX, yhi = -1;     // xlo / ylo over columns / rows >= 1 only
#pragma unroll 4
    for (long long p = threadIdx.x; p < hw; p += 1024) {
        float m = im[p];
        for (int c = 1; c < C; ++c) m = m + im[c * hw + p];
        if (m > 0.03f) {
            const int y = (int)(p / W), x = (int)(p - (long long)y * W);
            if (x >= 1) xlo = min(xlo, x);
            if (y >= 1) ylo = min(ylo, y);
            xhi = max(xhi, x);
            yhi = max(yhi, y);
        }
    }
    __shared__ int red[4][1024];
    red[0][threadIdx.x] = xlo; red[1][threadIdx.x] = xhi; red[2][threadIdx.x] = ylo; red[3][threadIdx.x] = yhi;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const int o = threadIdx.x + s;
            red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][o]);
            red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][o]);
            red[2][threadIdx.x] = min(red[2][threadIdx.x], red[2][o]);
            red[3][threadIdx.x] = max(red[3][threadIdx.x], red[3][o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float b0 = red[0][0] == INT_MAX ? 0.0f : (float)red[0][0];
        const float b1 = red[1][0] < 0 ? (float)W : (float)red[1][0];
        const float b2 = red[2][0] == INT_MAX ? 0.0f : (float)red[2][0];
        const float b3 = red[3][0] < 0 ? (float)H : (float)red[3][0];
        const float fw = (float)W, fh = (float)H;
        bounds[b * 4 + 0] = b0 / fw * 2.0f - 1.0f;
        bounds[b * 4 + 1] = b1 / fw * 2.0f - 1.0f;
        bounds[b * 4 + 2] = b2 / fh * 2.0f - 1.0f;
        bounds[b * 4 + 3] = b3 / fh * 2.0f - 1.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// per-sample extents (ext [B,4] = zmin, zmax, ymin, ymax; ext_idx the first vertex holding each) and the grid [B,N,2]
__global__ __launch_bounds__(1024) void gcn_extent_kernel(const float* __restrict__ verts,
                                                          const float* __restrict__ bounds, int N,
                                                          float* __restrict__ ext, int* __restrict__ ext_idx,
                                                          float* __restrict__ grid) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, t = threadIdx.x;
    const float* v = verts + (long long)b * N * 3;
    // (value, index) for zmin, zmax, ymin, ymax; ties keep the lower index
    float val[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    int idx[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    for (int i = t; i < N; i += 1024) {
        const float z = v[i * 3 + 2], y = v[i * 3 + 1];
        if (z < val[0]) { val[0] = z; idx[0] = i; }
        if (z > val[1]) { val[1] = z; idx[1] = i; }
        if (y < val[2]) { val[2] = y; idx[2] = i; }
        if (y > val[3]) { val[3] = y; idx[3] = i; }
    }
    __shared__ float sv[4][1024];
    __shared__ int si[4][1024];
#pragma unroll
    for (int k = 0; k < 4; ++k) { sv[k][t] = val[k]; si[k][t] = idx[k]; }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = sv[k][t], o = sv[k][t + s];
                const int ia = si[k][t], io = si[k][t + s];
                const bool better = (k & 1) ? (o > a) : (o < a);
                if (better || (o == a && io < ia)) { sv[k][t] = o; si[k][t] = io; }
            }
        }
        __syncthreads();
    }
    const float zmin = sv[0][0], zmax = sv[1][0], ymin = sv[2][0], ymax = sv[3][0];
    if (t < 4) {
        ext[b * 4 + t] = sv[t][0];
        ext_idx[b * 4 + t] = si[t][0] == INT_MAX ? 0 : si[t][0];
    }
    const float* bd = bounds + b * 4;
    const float b0 = bd[0], b1 = bd[1], b2 = bd[2], b3 = bd[3];
    for (int i = t; i < N; i += 1024) {
        const float z = v[i * 3 + 2], y = v[i * 3 + 1];
        // gcn.py:152-153, operation for operation
        const float gx = b0 + (1.0f - (z - zmin) / (zmax - zmin)) * (b1 - b0);
        const float gy = b2 + (1.0f - (y - ymin) / (ymax - ymin)) * (b3 - b2);
        grid[((long long)b * N + i) * 2 + 0] = gx;
        grid[((long long)b * N + i) * 2 + 1] = gy;
    }
}

// NCHW -> NHWC (forward, maps) or NHWC -> NCHW (backward, map gradients); one thread per destination element
template <bool TO_NHWC>
__global__ __launch_bounds__(256) void gcn_nhwc_kernel(GcnLevels lv, float* __restrict__ nhwc) {
    const int b = blockIdx.y;
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= lv.msize) return;
    int l = 0;
    while (l + 1 < lv.L && e >= lv.moff[l + 1]) ++l;
    const int r = e - lv.moff[l], C = lv.C[l], hw = lv.H[l] * lv.W[l];
    float* ws = nhwc + (long long)b * lv.msize + lv.moff[l];
    if (TO_NHWC) {                                  // r = p * C + c
        const int p = r / C, c = r - p * C;
        ws[r] = lv.map[l][((long long)b * C + c) * hw + p];
    } else {                                        // r = c * hw + p
        const int c = r / hw, p = r - c * hw;
        lv.dmap[l][(long long)b * C * hw + r] = ws[p * C + c];
    }
}

// bilinear corners of grid_sample (align_corners = True, zeros padding) for one level
struct Bilin {
    float ix, iy;
    int x0, y0;          // nw corner; valid only when `inside`
    bool inside;         // some corner may be in range (and ix / iy are finite)
};

__device__ inline Bilin bilin(float gx, float gy, int H, int W) {
#pragma clang fp contract(off)
    Bilin r;
    r.ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);   // grid_sampler_compute_source_index, align_corners
    r.iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    r.inside = r.ix > -1.0f && r.ix < (float)W && r.iy > -1.0f && r.iy < (float)H;    // false for NaN
    r.x0 = r.inside ? (int)floorf(r.ix) : 0;
    r.y0 = r.inside ? (int)floorf(r.iy) : 0;
    return r;
}

// conv1's input rows: one workgroup of 256 per vertex, coalesced row writes
__global__ __launch_bounds__(256) void gcn_input_kernel(const float* __restrict__ verts,
                                                        const float* __restrict__ grid,
                                                        const float* __restrict__ nhwc,
                                                        const float* __restrict__ glob, GcnLevels lv, int N,
                                                        int venc, int G, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long row = blockIdx.x;
    const int b = (int)(row / N);
    const int ctot = venc + lv.ctot_pool + G;
    float* o = out + row * ctot;
    for (int c = threadIdx.x; c < ctot; c += 256) {
        float val;
        if (c < venc) {
            if (c < 3) val = verts[row * 3 + c];
            else {                                   // [x, sin(x), cos(x), sin(2x), ..., cos(32x)], 3 channels each
                const int k = (c - 3) / 3, d = c - 3 - k * 3;
                const float a = verts[row * 3 + d] * (float)(1 << (k >> 1));
                val = (k & 1) ? cosf(a) : sinf(a);
            }
        } else if (c < venc + lv.ctot_pool) {
            const int cp = c - venc;
            int l = 0;
            while (l + 1 < lv.L && cp >= lv.coff[l + 1]) ++l;
            const int cl = cp - lv.coff[l], H = lv.H[l], W = lv.W[l], C = lv.C[l];
            const Bilin q = bilin(grid[row * 2], grid[row * 2 + 1], H, W);
            val = 0.0f;
            if (q.inside) {
                const float* m = nhwc + (long long)b * lv.msize + lv.moff[l];
                const int x1 = q.x0 + 1, y1 = q.y0 + 1;
                const float fx1 = (float)x1 - q.ix, fx0 = q.ix - (float)q.x0;
                const float fy1 = (float)y1 - q.iy, fy0 = q.iy - (float)q.y0;
                const bool vx0 = q.x0 >= 0, vx1 = x1 < W, vy0 = q.y0 >= 0, vy1 = y1 < H;
                if (vx0 && vy0) val = val + m[(q.y0 * W + q.x0) * C + cl] * (fx1 * fy1);
                if (vx1 && vy0) val = val + m[(q.y0 * W + x1) * C + cl] * (fx0 * fy1);
                if (vx0 && vy1) val = val + m[(y1 * W + q.x0) * C + cl] * (fx1 * fy0);
                if (vx1 && vy1) val = val + m[(y1 * W + x1) * C + cl] * (fx0 * fy0);
            }
        } else {
            val = glob[(long long)b * G + (c - venc - lv.ctot_pool)];
        }
        o[c] = val;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward to the maps.  Cell of a vertex at a level: (x0 + 1, y0 + 1) in [0, W] x [0, H], or the sentinel cell
// (H + 1)(W + 1) when no corner is in range.  Keys (cell << 13 | vertex) are bitonic-sorted in LDS: the order inside a
// cell is the vertex order, so the result does not depend on scheduling.  cell_start[c] = first sorted slot of cell c;
// order[s] = (vertex bits, ix, iy) of sorted slot s, one 16-byte load for the gather below.
__global__ __launch_bounds__(1024) void gcn_pool_sort_kernel(const float* __restrict__ grid, GcnLevels lv, int N,
                                                             int P2, float4* __restrict__ order,
                                                             int* __restrict__ cell_start) {
    __shared__ unsigned keys[GCN_SORT_MAX_N];
    const int l = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int H = lv.H[l], W = lv.W[l];
    const unsigned ncell = (unsigned)(H + 1) * (W + 1);
    for (int i = t; i < P2; i += 1024) {
        unsigned k = 0xffffffffu;
        if (i < N) {
            const long long g = ((long long)b * N + i) * 2;
            const Bilin q = bilin(grid[g], grid[g + 1], H, W);
            const unsigned cell = q.inside ? (unsigned)((q.y0 + 1) * (W + 1) + (q.x0 + 1)) : ncell;
            k = (cell << GCN_SORT_VBITS) | (unsigned)i;
        }
        keys[i] = k;
    }
    __syncthreads();
    for (int size = 2; size <= P2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < P2; i += 1024) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned a = keys[i], c = keys[j];
                    const bool up = (i & size) == 0;
                    if ((a > c) == up) { keys[i] = c; keys[j] = a; }
                }
            }
            __syncthreads();
        }
    }
    float4* rec = order + ((long long)b * lv.L + l) * N;
    for (int i = t; i < N; i += 1024) {
        const int v = (int)(keys[i] & ((1u << GCN_SORT_VBITS) - 1));
        const long long g = ((long long)b * N + v) * 2;
        const Bilin q = bilin(grid[g], grid[g + 1], H, W);
        rec[i] = make_float4(__int_as_float(v), q.ix, q.iy, 0.0f);
    }
    int* cs = cell_start + (long long)b * lv.cs_size + lv.cstart[l];
    for (unsigned c = t; c <= ncell; c += 1024) {       // lower bound of (c << 13) among the N real keys
        const unsigned key = c << GCN_SORT_VBITS;
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        cs[c] = lo;
    }
}

// one workgroup per (sample, level, pixel, 64-channel chunk); wave k sums the vertices of the k-th neighbouring cell
// (4 independent partial sums for latency), the four waves are added in a fixed order: NHWC gradient in the workspace
__global__ __launch_bounds__(256) void gcn_pool_bwd_kernel(const float* __restrict__ g, const float4* __restrict__ order,
                                                           const int* __restrict__ cell_start, GcnLevels lv, int N,
                                                           int ctot, int venc, float* __restrict__ dnhwc) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    int blk = blockIdx.x, l = 0;
    for (; l < lv.L; ++l) {                         // block -> (level, pixel, chunk)
        const int nb = lv.H[l] * lv.W[l] * ((lv.C[l] + 63) / 64);
        if (blk < nb) break;
        blk -= nb;
    }
    if (l >= lv.L) return;                          // uniform per workgroup
    const int C = lv.C[l], W = lv.W[l], nch = (C + 63) / 64;
    const int p = blk / nch, c = (blk - p * nch) * 64 + (threadIdx.x & 63), y = p / W, x = p - y * W;
    const int k = threadIdx.x >> 6, dx = k & 1, dy = k >> 1;
    // pixel (x, y) is corner se / sw / ne / nw of vertices whose nw corner is (x-1, y-1) / (x, y-1) / (x-1, y) / (x, y),
    // i.e. of the vertices in cell (x + dx, y + dy)
    const float4* rec = order + ((long long)b * lv.L + l) * N;
    const int* cs = cell_start + (long long)b * lv.cs_size + lv.cstart[l];
    const int cell = (y + dy) * (W + 1) + (x + dx);
    const int s0 = cs[cell], s1 = cs[cell + 1];
    const bool live = c < C;
    const float* gb = g + (long long)b * N * ctot + venc + lv.coff[l] + (live ? c : 0);
    const float fx = (float)(x - 1 + dx), fy = (float)(y - 1 + dy);     // the vertices' x0, y0
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int s = s0;
    for (; s + 4 <= s1; s += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 r = rec[s + u];
            const float wx = dx ? (fx + 1.0f) - r.y : r.y - fx;      // this pixel is x0 (dx) or x0 + 1
            const float wy = dy ? (fy + 1.0f) - r.z : r.z - fy;
            acc[u] = acc[u] + gb[(long long)__float_as_int(r.x) * ctot] * (wx * wy);
        }
    }
    for (; s < s1; ++s) {
        const float4 r = rec[s];
        const float wx = dx ? (fx + 1.0f) - r.y : r.y - fx;
        const float wy = dy ? (fy + 1.0f) - r.z : r.z - fy;
        acc[0] = acc[0] + gb[(long long)__float_as_int(r.x) * ctot] * (wx * wy);
    }
    __shared__ float part[4][64];
    part[k][threadIdx.x & 63] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (k == 0 && live) {
        const int lane = threadIdx.x;
        dnhwc[(long long)b * lv.msize + lv.moff[l] + p * C + c] =
            ((part[3][lane] + part[2][lane]) + part[1][lane]) + part[0][lane];
    }
}

// one wave per vertex: d/d(vertex) through the encoding and through the grid (direct term), and per vertex the factor
// q = (dL/dgx * -(b1 - b0), dL/dgy * -(b3 - b2)) that the extent backward needs
__global__ __launch_bounds__(256) void gcn_vertex_bwd_kernel(const float* __restrict__ g,
                                                             const float* __restrict__ verts,
                                                             const float* __restrict__ bounds,
                                                             const float* __restrict__ ext,
                                                             const float* __restrict__ grid,
                                                             const float* __restrict__ nhwc, GcnLevels lv, int B, int N,
                                                             int ctot, int venc, float* __restrict__ qbuf,
                                                             float* __restrict__ dverts) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long long)B * N) return;
    const int b = (int)(row / N);
    const float* gr = g + row * ctot;
    float dx[3] = {0.0f, 0.0f, 0.0f};
    // encoding
    for (int c = lane; c < venc; c += 64) {
        const float gc = gr[c];
        if (c < 3) dx[c] += gc;
        else {
            const int k = (c - 3) / 3, d = c - 3 - k * 3;
            const float f = (float)(1 << (k >> 1));
            const float a = verts[row * 3 + d] * f;
            const float dd = (k & 1) ? -f * sinf(a) * gc : f * cosf(a) * gc;
            if (d == 0) dx[0] += dd; else if (d == 1) dx[1] += dd; else dx[2] += dd;
        }
    }
    // grid, summed over levels (grid_sampler_2d backward, zeros padding)
    float dgx = 0.0f, dgy = 0.0f;
    const float gxv = grid[row * 2], gyv = grid[row * 2 + 1];
    for (int l = 0; l < lv.L; ++l) {
        const int H = lv.H[l], W = lv.W[l], C = lv.C[l];
        const Bilin q = bilin(gxv, gyv, H, W);
        if (!q.inside) continue;
        const float* m = nhwc + (long long)b * lv.msize + lv.moff[l];
        const int x1 = q.x0 + 1, y1 = q.y0 + 1;
        const bool vx0 = q.x0 >= 0, vx1 = x1 < W, vy0 = q.y0 >= 0, vy1 = y1 < H;
        const float fx1 = (float)x1 - q.ix, fx0 = q.ix - (float)q.x0;
        const float fy1 = (float)y1 - q.iy, fy0 = q.iy - (float)q.y0;
        float gix = 0.0f, giy = 0.0f;
        for (int c = lane; c < C; c += 64) {
            const float go = gr[venc + lv.coff[l] + c];
            const float nw = (vx0 && vy0) ? m[(q.y0 * W + q.x0) * C + c] : 0.0f;
            const float ne = (vx1 && vy0) ? m[(q.y0 * W + x1) * C + c] : 0.0f;
            const float sw = (vx0 && vy1) ? m[(y1 * W + q.x0) * C + c] : 0.0f;
            const float se = (vx1 && vy1) ? m[(y1 * W + x1) * C + c] : 0.0f;
            gix += ((ne - nw) * fy1 + (se - sw) * fy0) * go;
            giy += ((sw - nw) * fx1 + (se - ne) * fx0) * go;
        }
        dgx += gix * ((float)(W - 1) * 0.5f);
        dgy += giy * ((float)(H - 1) * 0.5f);
    }
    dgx = wave_sum(dgx);
    dgy = wave_sum(dgy);
    dx[0] = wave_sum(dx[0]);
    dx[1] = wave_sum(dx[1]);
    dx[2] = wave_sum(dx[2]);
    if (lane == 0 && lv.L == 0) {
        dverts[row * 3 + 0] = dx[0];
        dverts[row * 3 + 1] = dx[1];
        dverts[row * 3 + 2] = dx[2];
    } else if (lane == 0) {
        const float* bd = bounds + b * 4;
        const float* e = ext + b * 4;
        const float qx = dgx * -(bd[1] - bd[0]), qy = dgy * -(bd[3] - bd[2]);
        qbuf[row * 2] = qx;
        qbuf[row * 2 + 1] = qy;
        dverts[row * 3 + 0] = dx[0];
        dverts[row * 3 + 1] = dx[1] + qy / (e[3] - e[2]);
        dverts[row * 3 + 2] = dx[2] + qx / (e[1] - e[0]);
    }
}

// t = (z - m) / (M - m): dt/dm = (z - M) / D^2, dt/dM = -(z - m) / D^2; the sums go to the arg-extreme vertices
__global__ __launch_bounds__(256) void gcn_extent_bwd_kernel(const float* __restrict__ verts,
                                                             const float* __restrict__ ext,
                                                             const int* __restrict__ ext_idx,
                                                             const float* __restrict__ qbuf, int N,
                                                             float* __restrict__ dverts) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* e = ext + b * 4;
    const float zmin = e[0], zmax = e[1], ymin = e[2], ymax = e[3];
    const float dz = zmax - zmin, dy = ymax - ymin;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = t; i < N; i += 256) {
        const long long row = (long long)b * N + i;
        const float z = verts[row * 3 + 2], y = verts[row * 3 + 1];
        const float qx = qbuf[row * 2], qy = qbuf[row * 2 + 1];
        s[0] += qx * (z - zmax);
        s[1] -= qx * (z - zmin);
        s[2] += qy * (y - ymax);
        s[3] -= qy * (y - ymin);
    }
    __shared__ float red[4][256];
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][t] = s[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        float* dv = dverts + (long long)b * N * 3;
        const int* ix = ext_idx + b * 4;
        dv[ix[0] * 3 + 2] += red[0][0] / (dz * dz);
        dv[ix[1] * 3 + 2] += red[1][0] / (dz * dz);
        dv[ix[2] * 3 + 1] += red[2][0] / (dy * dy);
        dv[ix[3] * 3 + 1] += red[3][0] / (dy * dy);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// conv1 in factored form: h = x Theta without x.  proj [B, sum H_l W_l, Cout] holds the projected maps
// P_l = map_l(NHWC) Theta_l, level after level (a GcnLevels with C[l] = Cout, coff[l] = 0), gtheta [B, Cout] = g Theta_g,
// theta_e [venc, Cout] the encoding rows of Theta.
constexpr int GCNF_TV = 32;              // vertices per workgroup of the forward
constexpr int GCNF_CH = 128;             // channels per workgroup of the forward: 32 lanes of dwordx4 per vertex
constexpr int GCNF_ENC = 39;             // widest encoding
constexpr int GCNF_ENC_LD = 40;
constexpr int GCNF_ENC_ROWS = 128;       // rows per partial sum of dTheta_e
constexpr int GCNF_BT = 16;              // vertices per workgroup of the vertex backward
constexpr int GCNF_BC = 512;             // channels per pass of the vertex backward: 4 waves x 64 lanes x 2

// channel k of the encoding of vertex v3 (venc = 3: the vertex itself), as gcn_input_kernel forms it
__device__ inline float gcn_enc(const float* v3, int k) {
    if (k < 3) return v3[k];
    const int kk = (k - 3) / 3, d = k - 3 - kk * 3;
    const float a = v3[d] * (float)(1 << (kk >> 1));
    return (kk & 1) ? cosf(a) : sinf(a);
}

// d enc_k / d v3[k % 3]
__device__ inline float gcn_enc_deriv(const float* v3, int k) {
    if (k < 3) return 1.0f;
    const int kk = (k - 3) / 3, d = k - 3 - kk * 3;
    const float f = (float)(1 << (kk >> 1));
    const float a = v3[d] * f;
    return (kk & 1) ? -f * sinf(a) : f * cosf(a);
}

// h[b,v,c] = sum_k enc_k(v) Theta_e[k,c] + sum_l sum_corner w P_l[b,pix,c] + gTheta[b,c], summed in that order (corners
// nw, ne, sw, se).  One workgroup per (32 vertices, 128 channels, sample): Theta_e's chunk and the tile's encodings in LDS,
// then 32 lanes per vertex, each with 4 channels: every corner is one 512-byte run of dwordx4 loads.
__global__ __launch_bounds__(256) void gcn_factored_fwd_kernel(const float* __restrict__ verts,
                                                               const float* __restrict__ grid,
                                                               const float* __restrict__ proj,
                                                               const float* __restrict__ gtheta,
                                                               const float* __restrict__ theta_e, GcnLevels lv, int N,
                                                               int venc, int Cout, float* __restrict__ out) {
    __shared__ float s_th[GCNF_ENC * GCNF_CH] __attribute__((aligned(16)));
    __shared__ float s_enc[GCNF_TV * GCNF_ENC_LD];
    const int b = blockIdx.z, c0 = blockIdx.y * GCNF_CH, v0 = blockIdx.x * GCNF_TV, t = threadIdx.x;
    for (int i = t; i < venc * GCNF_CH; i += 256) {
        const int k = i / GCNF_CH, c = i - k * GCNF_CH;
        s_th[i] = c0 + c < Cout ? theta_e[(long long)k * Cout + c0 + c] : 0.0f;
    }
    for (int i = t; i < GCNF_TV * venc; i += 256) {
        const int vi = i / venc, k = i - vi * venc, v = v0 + vi;
        s_enc[vi * GCNF_ENC_LD + k] = v < N ? gcn_enc(verts + ((long long)b * N + v) * 3, k) : 0.0f;
    }
    __syncthreads();
    const int q = t & 31, c = c0 + q * 4;
    if (c >= Cout) return;                                  // after the only barrier
    for (int vi = t >> 5; vi < GCNF_TV; vi += 8) {
        const int v = v0 + vi;
        if (v >= N) break;
        const long long row = (long long)b * N + v;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < venc; ++k) {
            const float e = s_enc[vi * GCNF_ENC_LD + k];
            const float4 th = *reinterpret_cast<const float4*>(&s_th[k * GCNF_CH + q * 4]);
            acc[0] = fmaf(e, th.x, acc[0]); acc[1] = fmaf(e, th.y, acc[1]);
            acc[2] = fmaf(e, th.z, acc[2]); acc[3] = fmaf(e, th.w, acc[3]);
        }
        if (lv.L > 0) {
            const float gx = grid[row * 2], gy = grid[row * 2 + 1];
            for (int l = 0; l < lv.L; ++l) {
                const int H = lv.H[l], W = lv.W[l];
                const Bilin qd = bilin(gx, gy, H, W);
                if (!qd.inside) continue;
                const float* m = proj + (long long)b * lv.msize + lv.moff[l] + c;
                const int x1 = qd.x0 + 1, y1 = qd.y0 + 1;
                const bool vx0 = qd.x0 >= 0, vx1 = x1 < W, vy0 = qd.y0 >= 0, vy1 = y1 < H;
                float wnw, wne, wsw, wse;
                {
#pragma clang fp contract(off)
                    const float fx1 = (float)x1 - qd.ix, fx0 = qd.ix - (float)qd.x0;
                    const float fy1 = (float)y1 - qd.iy, fy0 = qd.iy - (float)qd.y0;
                    wnw = fx1 * fy1; wne = fx0 * fy1; wsw = fx1 * fy0; wse = fx0 * fy0;
                }
                // all four loads go out together from addresses clamped into the map; a corner outside it is not added
                const int xa = vx0 ? qd.x0 : 0, xb = vx1 ? x1 : W - 1, ya = vy0 ? qd.y0 : 0, yb = vy1 ? y1 : H - 1;
                const float4 pnw = *reinterpret_cast<const float4*>(m + (long long)(ya * W + xa) * Cout);
                const float4 pne = *reinterpret_cast<const float4*>(m + (long long)(ya * W + xb) * Cout);
                const float4 psw = *reinterpret_cast<const float4*>(m + (long long)(yb * W + xa) * Cout);
                const float4 pse = *reinterpret_cast<const float4*>(m + (long long)(yb * W + xb) * Cout);
                if (vx0 && vy0) {
                    acc[0] = fmaf(wnw, pnw.x, acc[0]); acc[1] = fmaf(wnw, pnw.y, acc[1]);
                    acc[2] = fmaf(wnw, pnw.z, acc[2]); acc[3] = fmaf(wnw, pnw.w, acc[3]);
                }
                if (vx1 && vy0) {
                    acc[0] = fmaf(wne, pne.x, acc[0]); acc[1] = fmaf(wne, pne.y, acc[1]);
                    acc[2] = fmaf(wne, pne.z, acc[2]); acc[3] = fmaf(wne, pne.w, acc[3]);
                }
                if (vx0 && vy1) {
                    acc[0] = fmaf(wsw, psw.x, acc[0]); acc[1] = fmaf(wsw, psw.y, acc[1]);
                    acc[2] = fmaf(wsw, psw.z, acc[2]); acc[3] = fmaf(wsw, psw.w, acc[3]);
                }
                if (vx1 && vy1) {
                    acc[0] = fmaf(wse, pse.x, acc[0]); acc[1] = fmaf(wse, pse.y, acc[1]);
                    acc[2] = fmaf(wse, pse.z, acc[2]); acc[3] = fmaf(wse, pse.w, acc[3]);
                }
            }
        }
        if (gtheta) {
            const float4 gt = *reinterpret_cast<const float4*>(gtheta + (long long)b * Cout + c);
            acc[0] += gt.x; acc[1] += gt.y; acc[2] += gt.z; acc[3] += gt.w;
        }
        *reinterpret_cast<float4*>(out + row * Cout + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// dTheta_e[k,c] = sum_rows enc_k(row) g[row,c] in a fixed order, in the pattern of gcn_colsum_*: partial sums over chunks of
// 128 rows, then the chunks in order.  One workgroup per (64 channels, chunk): the chunk's encodings in LDS (rows of 40,
// read four at a time), one thread per channel with the 39 running sums in registers; wave w takes rows w, w + 4, ... and
// the four waves are added in a fixed order through LDS (the encodings' space, once every wave has read them).
__global__ __launch_bounds__(256) void gcn_factored_enc_partial_kernel(const float* __restrict__ g,
                                                                       const float* __restrict__ verts, long long rows,
                                                                       int venc, int Cout, float* __restrict__ ws) {
    __shared__ float s_buf[3 * GCNF_ENC * 64] __attribute__((aligned(16)));
    static_assert(3 * GCNF_ENC * 64 >= GCNF_ENC_ROWS * GCNF_ENC_LD, "the encodings of a chunk fit");
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, c = blockIdx.x * 64 + lane, p = blockIdx.y;
    const long long r0 = (long long)p * GCNF_ENC_ROWS;
    const int nr = (int)(rows - r0 < GCNF_ENC_ROWS ? rows - r0 : GCNF_ENC_ROWS);
    for (int i = t; i < GCNF_ENC_ROWS * GCNF_ENC_LD; i += 256) {
        const int r = i / GCNF_ENC_LD, k = i - r * GCNF_ENC_LD;
        s_buf[i] = (r < nr && k < venc) ? gcn_enc(verts + (r0 + r) * 3, k) : 0.0f;
    }
    __syncthreads();
    const bool live = c < Cout;
    float acc[GCNF_ENC_LD];                                 // entry 39 pairs with the rows' zero padding
#pragma unroll
    for (int k = 0; k < GCNF_ENC_LD; ++k) acc[k] = 0.0f;
    for (int r = w; r < nr; r += 16) {                     // four rows' gradients in flight; rows past nr are zeros in LDS
        float gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = (live && r + 4 * u < nr) ? g[(r0 + r + 4 * u) * Cout + c] : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int k4 = 0; k4 < GCNF_ENC_LD / 4; ++k4) {
                const float4 e = *reinterpret_cast<const float4*>(&s_buf[(r + 4 * u) * GCNF_ENC_LD + k4 * 4]);
                acc[k4 * 4 + 0] = fmaf(e.x, gv[u], acc[k4 * 4 + 0]); acc[k4 * 4 + 1] = fmaf(e.y, gv[u], acc[k4 * 4 + 1]);
                acc[k4 * 4 + 2] = fmaf(e.z, gv[u], acc[k4 * 4 + 2]); acc[k4 * 4 + 3] = fmaf(e.w, gv[u], acc[k4 * 4 + 3]);
            }
        }
    }
    __syncthreads();
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < GCNF_ENC; ++k) s_buf[((w - 1) * GCNF_ENC + k) * 64 + lane] = acc[k];
    }
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
        for (int k = 0; k < GCNF_ENC; ++k)
            if (k < venc)
                ws[((long long)p * venc + k) * Cout + c] =
                    ((acc[k] + s_buf[(0 * GCNF_ENC + k) * 64 + lane]) + s_buf[(1 * GCNF_ENC + k) * 64 + lane]) +
                    s_buf[(2 * GCNF_ENC + k) * 64 + lane];
    }
}

__global__ __launch_bounds__(256) void gcn_factored_enc_final_kernel(const float* __restrict__ ws, int n, int P,
                                                                     float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int p = 0; p < P; ++p) acc += ws[(long long)p * n + i];
    out[i] = acc;
}

// d/d(vertex) from g = dh: the encoding term g Theta_e^T d enc, and the grid term of gcn_vertex_bwd_kernel with the
// projected maps in place of the maps and g in place of the per-level columns.  One workgroup per 16 vertices; wave w and
// lane i own channels 128 w + 2 i (+ 512 per pass), with Theta_e's 39 x 2 entries in registers for the whole tile; the
// five sums of a vertex are reduced per wave, then over the four waves in a fixed order.
__global__ __launch_bounds__(256) void gcn_factored_vertex_bwd_kernel(const float* __restrict__ g,
                                                                      const float* __restrict__ verts,
                                                                      const float* __restrict__ bounds,
                                                                      const float* __restrict__ ext,
                                                                      const float* __restrict__ grid,
                                                                      const float* __restrict__ proj,
                                                                      const float* __restrict__ theta_e, GcnLevels lv,
                                                                      int B, int N, int venc, int Cout,
                                                                      float* __restrict__ qbuf,
                                                                      float* __restrict__ dverts) {
    __shared__ float s_der[GCNF_BT * GCNF_ENC_LD];
    __shared__ float s_part[4 * GCNF_BT * 5];
    const long long rows = (long long)B * N, r0 = (long long)blockIdx.x * GCNF_BT;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int i = t; i < GCNF_BT * GCNF_ENC_LD; i += 256) {
        const int vi = i / GCNF_ENC_LD, k = i - vi * GCNF_ENC_LD;
        s_der[i] = (k < venc && r0 + vi < rows) ? gcn_enc_deriv(verts + (r0 + vi) * 3, k) : 0.0f;
    }
    for (int i = t; i < 4 * GCNF_BT * 5; i += 256) s_part[i] = 0.0f;
    __syncthreads();
    for (int cp = 0; cp < Cout; cp += GCNF_BC) {
        const int c = cp + w * 128 + lane * 2;
        const bool live = c < Cout;                         // Cout is even: c + 1 is a channel when c is
        float th[GCNF_ENC][2];
#pragma unroll
        for (int k = 0; k < GCNF_ENC; ++k) {
            const bool on = live && k < venc;
            th[k][0] = on ? theta_e[(long long)k * Cout + c] : 0.0f;
            th[k][1] = on ? theta_e[(long long)k * Cout + c + 1] : 0.0f;
        }
        for (int vi = 0; vi < GCNF_BT; ++vi) {
            const long long row = r0 + vi;
            if (row >= rows) break;                         // uniform per workgroup
            const int b = (int)(row / N);
            const float* gr = g + row * Cout + c;
            const float g0 = live ? gr[0] : 0.0f, g1 = live ? gr[1] : 0.0f;
            float td[3][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
            for (int k = 0; k < GCNF_ENC; ++k) {
                const float dk = s_der[vi * GCNF_ENC_LD + k];
                td[k % 3][0] = fmaf(dk, th[k][0], td[k % 3][0]);
                td[k % 3][1] = fmaf(dk, th[k][1], td[k % 3][1]);
            }
            float s[5];
            s[0] = g0 * td[0][0] + g1 * td[0][1];
            s[1] = g0 * td[1][0] + g1 * td[1][1];
            s[2] = g0 * td[2][0] + g1 * td[2][1];
            s[3] = 0.0f; s[4] = 0.0f;
            if (lv.L > 0) {
                const float gxv = grid[row * 2], gyv = grid[row * 2 + 1];
                for (int l = 0; l < lv.L; ++l) {
                    const int H = lv.H[l], W = lv.W[l];
                    const Bilin q = bilin(gxv, gyv, H, W);
                    if (!q.inside || !live) continue;
                    const float* m = proj + (long long)b * lv.msize + lv.moff[l] + c;
                    const int x1 = q.x0 + 1, y1 = q.y0 + 1;
                    const bool vx0 = q.x0 >= 0, vx1 = x1 < W, vy0 = q.y0 >= 0, vy1 = y1 < H;
                    const float fx1 = (float)x1 - q.ix, fx0 = q.ix - (float)q.x0;
                    const float fy1 = (float)y1 - q.iy, fy0 = q.iy - (float)q.y0;
                    float gix = 0.0f, giy = 0.0f;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float go = j ? g1 : g0;
                        const float nw = (vx0 && vy0) ? m[(long long)(q.y0 * W + q.x0) * Cout + j] : 0.0f;
                        const float ne = (vx1 && vy0) ? m[(long long)(q.y0 * W + x1) * Cout + j] : 0.0f;
                        const float sw = (vx0 && vy1) ? m[(long long)(y1 * W + q.x0) * Cout + j] : 0.0f;
                        const float se = (vx1 && vy1) ? m[(long long)(y1 * W + x1) * Cout + j] : 0.0f;
                        gix += ((ne - nw) * fy1 + (se - sw) * fy0) * go;
                        giy += ((sw - nw) * fx1 + (se - ne) * fx0) * go;
                    }
                    s[3] += gix * ((float)(W - 1) * 0.5f);
                    s[4] += giy * ((float)(H - 1) * 0.5f);
                }
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) s[j] = wave_sum(s[j]);
            if (lane == 0) {                                // this wave's own slots: passes add up in order
#pragma unroll
                for (int j = 0; j < 5; ++j) s_part[(w * GCNF_BT + vi) * 5 + j] += s[j];
            }
        }
    }
    __syncthreads();
    if (t < GCNF_BT && r0 + t < rows) {
        const long long row = r0 + t;
        float s[5];
#pragma unroll
        for (int j = 0; j < 5; ++j)
            s[j] = ((s_part[(0 * GCNF_BT + t) * 5 + j] + s_part[(1 * GCNF_BT + t) * 5 + j]) +
                    s_part[(2 * GCNF_BT + t) * 5 + j]) + s_part[(3 * GCNF_BT + t) * 5 + j];
        if (lv.L == 0) {
            dverts[row * 3 + 0] = s[0];
            dverts[row * 3 + 1] = s[1];
            dverts[row * 3 + 2] = s[2];
        } else {
            const int b = (int)(row / N);
            const float* bd = bounds + b * 4;
            const float* e = ext + b * 4;
            const float qx = s[3] * -(bd[1] - bd[0]), qy = s[4] * -(bd[3] - bd[2]);
            qbuf[row * 2] = qx;
            qbuf[row * 2 + 1] = qy;
            dverts[row * 3 + 0] = s[0];
            dverts[row * 3 + 1] = s[1] + qy / (e[3] - e[2]);
            dverts[row * 3 + 2] = s[2] + qx / (e[1] - e[0]);
        }
    }
}

}  // namespace vpn

using namespace vpn;

static int gcn_levels(int L, const float* f0, const float* f1, const float* f2, const float* f3, int C0, int H0, int W0,
                      int C1, int H1, int W1, int C2, int H2, int W2, int C3, int H3, int W3, GcnLevels* lv) {
    if (L < 0 || L > GCN_MAX_LEVELS) return VPN_E_BADARG;
    const float* m[4] = {f0, f1, f2, f3};
    const int C[4] = {C0, C1, C2, C3}, H[4] = {H0, H1, H2, H3}, W[4] = {W0, W1, W2, W3};
    long long coff = 0, moff = 0, cs = 0;
    *lv = GcnLevels{};
    lv->L = L;
    long long blocks = 0;
    for (int l = 0; l < L; ++l) {
        if (C[l] <= 0 || H[l] <= 0 || W[l] <= 0) return VPN_E_BADARG;
        if ((long long)H[l] * W[l] > (1 << 24)) return VPN_E_TOOBIG;
        blocks += (long long)H[l] * W[l] * ((C[l] + 63) / 64);
        if (blocks > 0x7fffffffLL) return VPN_E_TOOBIG;
        lv->map[l] = m[l];
        lv->C[l] = C[l]; lv->H[l] = H[l]; lv->W[l] = W[l];
        lv->coff[l] = (int)coff; lv->moff[l] = (int)moff; lv->cstart[l] = (int)cs;
        coff += C[l];
        moff += (long long)C[l] * H[l] * W[l];
        cs += (long long)(H[l] + 1) * (W[l] + 1) + 2;
        if (moff > 0x7fffffffLL || cs > 0x7fffffffLL) return VPN_E_TOOBIG;
    }
    lv->ctot_pool = (int)coff;
    lv->msize = (int)moff;
    lv->cs_size = (int)cs;
    return 0;
}

extern "C" int vpn_gcn_aggregate(const float* x, const int32_t* row_ptr, const int32_t* col, const float* w,
                                 const float* bias, const float* mask, int B, int N, int C, int relu, float* out,
                                 void* stream) {
    if (!x || !row_ptr || !col || !w || !out || B <= 0 || N <= 0 || C <= 0) return VPN_E_BADARG;
    const long long rows = (long long)B * N;
    if (rows * C > 0x7fffffffLL * 4) return VPN_E_TOOBIG;
    const bool v4 = (C % 4) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                    (!mask || ((uintptr_t)mask % 16) == 0);
    const long long total = rows * (v4 ? C / 4 : C);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (v4)
        VPN_LAUNCH_AS("gcn_aggregate_kernel", gcn_aggregate_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x,
                      row_ptr, col, w, bias, mask, N, C, relu, total, out);
    else
        VPN_LAUNCH_AS("gcn_aggregate_kernel", gcn_aggregate_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x,
                      row_ptr, col, w, bias, mask, N, C, relu, total, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vpn_gcn_colsum_workspace(int S, int R, int C) {
    if (S <= 0 || R <= 0 || C <= 0) return 0;
    return (size_t)S * ((R + GCN_COLSUM_ROWS - 1) / GCN_COLSUM_ROWS) * C * sizeof(float);
}

extern "C" int vpn_gcn_colsum(const float* in, const float* mask, int S, int R, int ld, int off, int C, void* workspace,
                              float* out, void* stream) {
    if (!in || !workspace || !out || S <= 0 || R <= 0 || C <= 0 || off < 0 || ld < off + C) return VPN_E_BADARG;
    if ((long long)S * R * ld > 0x7fffffffLL * 4) return VPN_E_TOOBIG;
    const int P = (R + GCN_COLSUM_ROWS - 1) / GCN_COLSUM_ROWS;
    if (P > 65535 || S > 65535) return VPN_E_TOOBIG;
    float* ws = (float*)workspace;
    VPN_LAUNCH(gcn_colsum_partial_kernel, dim3((C + 255) / 256, P, S), dim3(256), 0, (hipStream_t)stream, in, mask, R,
               ld, off, C, P, ws);
    VPN_LAUNCH(gcn_colsum_final_kernel, dim3((C + 255) / 256, S), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
               C, P, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_gcn_bounds(const float* img, int B, int C, int H, int W, float* bounds, void* stream) {
    if (!img || !bounds || B <= 0 || C <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    if ((long long)C * H * W > 0x7fffffffLL) return VPN_E_TOOBIG;
    VPN_LAUNCH(gcn_bounds_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, img, C, H, W, bounds);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vpn_gcn_maps_workspace(int B, int L, int C0, int H0, int W0, int C1, int H1, int W1, int C2, int H2,
                                         int W2, int C3, int H3, int W3) {
    GcnLevels lv;
    if (B <= 0 || gcn_levels(L, nullptr, nullptr, nullptr, nullptr, C0, H0, W0, C1, H1, W1, C2, H2, W2, C3, H3, W3, &lv))
        return 0;
    return (size_t)B * lv.msize * sizeof(float);
}

extern "C" int vpn_gcn_input_fwd(const float* verts, const float* bounds, const float* glob, int B, int N, int G,
                                 int venc, int L, const float* f0, const float* f1, const float* f2, const float* f3,
                                 int C0, int H0, int W0, int C1, int H1, int W1, int C2, int H2, int W2, int C3, int H3,
                                 int W3, float* ext, int32_t* ext_idx, float* grid, void* maps_ws, float* out,
                                 void* stream) {
    if (!verts || !out || B <= 0 || N <= 0 || G < 0 || (G > 0 && !glob)) return VPN_E_BADARG;
    if (venc != 0 && venc != 3 && venc != 39) return VPN_E_BADARG;
    GcnLevels lv;
    int rc = gcn_levels(L, f0, f1, f2, f3, C0, H0, W0, C1, H1, W1, C2, H2, W2, C3, H3, W3, &lv);
    if (rc) return rc;
    for (int l = 0; l < L; ++l)
        if (!lv.map[l]) return VPN_E_BADARG;
    if (L > 0 && (!bounds || !ext || !ext_idx || !grid || !maps_ws)) return VPN_E_BADARG;
    const long long ctot = (long long)venc + lv.ctot_pool + G;
    if (ctot <= 0) return VPN_E_BADARG;
    if ((long long)B * N > 0x7fffffffLL || (long long)B * N * ctot > 0x7fffffffLL * 4 || B > 65535) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (L > 0) {
        VPN_LAUNCH(gcn_extent_kernel, dim3(B), dim3(1024), 0, s, verts, bounds, N, ext, (int*)ext_idx, grid);
        VPN_LAUNCH_AS("gcn_nhwc_kernel", gcn_nhwc_kernel<true>, dim3((lv.msize + 255) / 256, B), dim3(256), 0, s, lv,
                      (float*)maps_ws);
    }
    VPN_LAUNCH(gcn_input_kernel, dim3((unsigned)((long long)B * N)), dim3(256), 0, s, verts, (const float*)grid,
               (const float*)maps_ws, glob, lv, N, venc, G, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

// workspace of vpn_gcn_input_bwd: sorted records [B,L,N] float4, cell starts [B, cs_size] int, q [B,N,2], NHWC gradient
// [B, msize]
static size_t gcn_bwd_ws(int B, int N, const GcnLevels& lv) {
    return ((size_t)B * lv.L * N * 4 + (size_t)B * lv.cs_size + (size_t)B * N * 2 + (size_t)B * lv.msize) * 4;
}

extern "C" size_t vpn_gcn_input_bwd_workspace(int B, int N, int L, int C0, int H0, int W0, int C1, int H1, int W1,
                                              int C2, int H2, int W2, int C3, int H3, int W3) {
    GcnLevels lv;
    if (B <= 0 || N <= 0 ||
        gcn_levels(L, nullptr, nullptr, nullptr, nullptr, C0, H0, W0, C1, H1, W1, C2, H2, W2, C3, H3, W3, &lv))
        return 0;
    return gcn_bwd_ws(B, N, lv);
}

extern "C" int vpn_gcn_input_bwd(const float* grad, const float* verts, const float* bounds, int B, int N, int G,
                                 int venc, int L, int C0, int H0, int W0, int C1, int H1, int W1, int C2, int H2,
                                 int W2, int C3, int H3, int W3, const float* ext, const int32_t* ext_idx,
                                 const float* grid, const void* maps_ws, void* workspace, float* grad_verts,
                                 float* gf0, float* gf1, float* gf2, float* gf3, void* stream) {
    if (!grad || !verts || B <= 0 || N <= 0 || G < 0) return VPN_E_BADARG;
    if (venc != 0 && venc != 3 && venc != 39) return VPN_E_BADARG;
    GcnLevels lv;
    int rc = gcn_levels(L, nullptr, nullptr, nullptr, nullptr, C0, H0, W0, C1, H1, W1, C2, H2, W2, C3, H3, W3, &lv);
    if (rc) return rc;
    float* gf[4] = {gf0, gf1, gf2, gf3};
    bool any_map = false;
    for (int l = 0; l < L; ++l) { lv.dmap[l] = gf[l]; any_map |= gf[l] != nullptr; }
    for (int l = 0; l < L; ++l)
        if (any_map && !gf[l]) return VPN_E_BADARG;         // all levels or none
    if (L > 0 && (!bounds || !ext || !ext_idx || !grid || !maps_ws || !workspace)) return VPN_E_BADARG;
    const long long ctot = (long long)venc + lv.ctot_pool + G;
    if ((long long)B * N > 0x7fffffffLL || (long long)B * N * ctot > 0x7fffffffLL * 4 || B > 65535) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    float4* order = (float4*)workspace;
    int* cstart = (int*)(order + (size_t)B * L * N);
    float* qbuf = (float*)(cstart + (size_t)B * lv.cs_size);
    float* dnhwc = qbuf + (size_t)B * N * 2;
    if (any_map && L > 0) {
        if (N > GCN_SORT_MAX_N) return VPN_E_TOOBIG;
        for (int l = 0; l < L; ++l)
            if ((long long)(lv.H[l] + 1) * (lv.W[l] + 1) >= (1LL << (32 - GCN_SORT_VBITS)) - 1) return VPN_E_TOOBIG;
        int P2 = 1;
        while (P2 < N) P2 <<= 1;
        VPN_LAUNCH(gcn_pool_sort_kernel, dim3(L, B), dim3(1024), 0, s, grid, lv, N, P2, order, cstart);
        int nblk = 0;
        for (int l = 0; l < L; ++l) nblk += lv.H[l] * lv.W[l] * ((lv.C[l] + 63) / 64);
        VPN_LAUNCH(gcn_pool_bwd_kernel, dim3(nblk, B), dim3(256), 0, s, grad, (const float4*)order,
                   (const int*)cstart, lv, N, (int)ctot, venc, dnhwc);
        VPN_LAUNCH_AS("gcn_nhwc_kernel", gcn_nhwc_kernel<false>, dim3((lv.msize + 255) / 256, B), dim3(256), 0, s, lv,
                      dnhwc);
    }
    if (grad_verts) {
        const long long rows = (long long)B * N;
        VPN_LAUNCH(gcn_vertex_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, grad, verts, bounds, ext,
                   grid, (const float*)maps_ws, lv, B, N, (int)ctot, venc, qbuf, grad_verts);
        if (L > 0)
            VPN_LAUNCH(gcn_extent_bwd_kernel, dim3(B), dim3(256), 0, s, verts, ext, (const int*)ext_idx,
                       (const float*)qbuf, N, grad_verts);
    }
    VPN_LAUNCH_CHECK();
    return 0;
}

// ---- conv1 in factored form
// the levels of the projected maps: Cout channels each, every level reading the same gradient columns
static int gcnf_levels(int L, int Cout, int H0, int W0, int H1, int W1, int H2, int W2, int H3, int W3, GcnLevels* lv) {
    if (Cout <= 0 || (Cout % 4) != 0) return VPN_E_BADARG;
    const int rc = gcn_levels(L, nullptr, nullptr, nullptr, nullptr, Cout, H0, W0, Cout, H1, W1, Cout, H2, W2, Cout, H3, W3, lv);
    if (rc) return rc;
    for (int l = 0; l < L; ++l) lv->coff[l] = 0;
    return 0;
}

static bool gcnf_aligned(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" size_t vpn_gcn_factored_proj_workspace(int B, int Cout, int L, int H0, int W0, int H1, int W1, int H2, int W2,
                                                  int H3, int W3) {
    GcnLevels lv;
    if (B <= 0 || gcnf_levels(L, Cout, H0, W0, H1, W1, H2, W2, H3, W3, &lv)) return 0;
    return (size_t)B * lv.msize * sizeof(float);
}

extern "C" int vpn_gcn_factored_fwd(const float* verts, const float* bounds, const float* gtheta, const float* theta_e,
                                    const float* proj, int B, int N, int Cout, int venc, int L, int H0, int W0, int H1,
                                    int W1, int H2, int W2, int H3, int W3, float* ext, int32_t* ext_idx, float* grid,
                                    float* out, void* stream) {
    if (!verts || !out || B <= 0 || N <= 0) return VPN_E_BADARG;
    if (venc != 0 && venc != 3 && venc != 39) return VPN_E_BADARG;
    if (venc > 0 && !theta_e) return VPN_E_BADARG;
    GcnLevels lv;
    const int rc = gcnf_levels(L, Cout, H0, W0, H1, W1, H2, W2, H3, W3, &lv);
    if (rc) return rc;
    if (L > 0 && (!bounds || !ext || !ext_idx || !grid || !proj)) return VPN_E_BADARG;
    if (!gcnf_aligned(out) || !gcnf_aligned(proj) || !gcnf_aligned(gtheta) || !gcnf_aligned(theta_e)) return VPN_E_BADARG;
    if ((long long)B * N > 0x7fffffffLL || (long long)B * N * Cout > 0x7fffffffLL * 4 || B > 65535) return VPN_E_TOOBIG;
    const int cblk = (Cout + GCNF_CH - 1) / GCNF_CH;
    if (cblk > 65535) return VPN_E_TOOBIG;
    hipStream_t s = (hipStream_t)stream;
    if (L > 0) VPN_LAUNCH(gcn_extent_kernel, dim3(B), dim3(1024), 0, s, verts, bounds, N, ext, (int*)ext_idx, grid);
    VPN_LAUNCH(gcn_factored_fwd_kernel, dim3((N + GCNF_TV - 1) / GCNF_TV, cblk, B), dim3(256), 0, s, verts,
               (const float*)grid, proj, gtheta, theta_e, lv, N, venc, Cout, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

// workspace of vpn_gcn_factored_bwd: sorted records [B,L,N] float4, cell starts [B, cs_size] int, q [B,N,2], the partial
// sums of dTheta_e [ceil(B N / 128), venc, Cout]
static size_t gcnf_bwd_ws(int B, int N, int Cout, int venc, const GcnLevels& lv) {
    const size_t P = ((size_t)B * N + GCNF_ENC_ROWS - 1) / GCNF_ENC_ROWS;
    return ((size_t)B * lv.L * N * 4 + (size_t)B * lv.cs_size + (size_t)B * N * 2 + P * venc * Cout) * 4;
}

extern "C" size_t vpn_gcn_factored_bwd_workspace(int B, int N, int Cout, int venc, int L, int H0, int W0, int H1, int W1,
                                                 int H2, int W2, int H3, int W3) {
    GcnLevels lv;
    if (B <= 0 || N <= 0 || (venc != 0 && venc != 3 && venc != 39) ||
        gcnf_levels(L, Cout, H0, W0, H1, W1, H2, W2, H3, W3, &lv))
        return 0;
    return gcnf_bwd_ws(B, N, Cout, venc, lv);
}

extern "C" int vpn_gcn_factored_bwd(const float* grad, const float* verts, const float* bounds, const float* theta_e,
                                    const float* proj, int B, int N, int Cout, int venc, int L, int H0, int W0, int H1,
                                    int W1, int H2, int W2, int H3, int W3, const float* ext, const int32_t* ext_idx,
                                    const float* grid, void* workspace, float* grad_verts, float* grad_proj,
                                    float* grad_theta_e, void* stream) {
    if (!grad || !verts || B <= 0 || N <= 0) return VPN_E_BADARG;
    if (venc != 0 && venc != 3 && venc != 39) return VPN_E_BADARG;
    GcnLevels lv;
    const int rc = gcnf_levels(L, Cout, H0, W0, H1, W1, H2, W2, H3, W3, &lv);
    if (rc) return rc;
    const bool want_proj = grad_proj && L > 0, want_enc = grad_theta_e && venc > 0;
    if (!want_proj && !want_enc && !grad_verts) return 0;
    if (!workspace) return VPN_E_BADARG;
    if (L > 0 && (want_proj || grad_verts) && !grid) return VPN_E_BADARG;
    if (grad_verts && venc > 0 && !theta_e) return VPN_E_BADARG;
    if (grad_verts && L > 0 && (!bounds || !ext || !ext_idx || !proj)) return VPN_E_BADARG;
    if ((long long)B * N > 0x7fffffffLL || (long long)B * N * Cout > 0x7fffffffLL * 4 || B > 65535) return VPN_E_TOOBIG;
    const long long rows = (long long)B * N;
    hipStream_t s = (hipStream_t)stream;
    float4* order = (float4*)workspace;
    int* cstart = (int*)(order + (size_t)B * L * N);
    float* qbuf = (float*)(cstart + (size_t)B * lv.cs_size);
    float* encws = qbuf + (size_t)B * N * 2;
    if (want_proj) {
        if (N > GCN_SORT_MAX_N) return VPN_E_TOOBIG;
        for (int l = 0; l < L; ++l)
            if ((long long)(lv.H[l] + 1) * (lv.W[l] + 1) >= (1LL << (32 - GCN_SORT_VBITS)) - 1) return VPN_E_TOOBIG;
        int P2 = 1;
        while (P2 < N) P2 <<= 1;
        VPN_LAUNCH(gcn_pool_sort_kernel, dim3(L, B), dim3(1024), 0, s, grid, lv, N, P2, order, cstart);
        int nblk = 0;
        for (int l = 0; l < L; ++l) nblk += lv.H[l] * lv.W[l] * ((Cout + 63) / 64);
        VPN_LAUNCH(gcn_pool_bwd_kernel, dim3(nblk, B), dim3(256), 0, s, grad, (const float4*)order, (const int*)cstart,
                   lv, N, Cout, 0, grad_proj);
    }
    if (want_enc) {
        const long long P = (rows + GCNF_ENC_ROWS - 1) / GCNF_ENC_ROWS;
        if (P > 65535) return VPN_E_TOOBIG;
        VPN_LAUNCH(gcn_factored_enc_partial_kernel, dim3((Cout + 63) / 64, (unsigned)P), dim3(256), 0, s, grad, verts,
                   rows, venc, Cout, encws);
        VPN_LAUNCH(gcn_factored_enc_final_kernel, dim3((venc * Cout + 255) / 256), dim3(256), 0, s, (const float*)encws,
                   venc * Cout, (int)P, grad_theta_e);
    }
    if (grad_verts) {
        VPN_LAUNCH(gcn_factored_vertex_bwd_kernel, dim3((unsigned)((rows + GCNF_BT - 1) / GCNF_BT)), dim3(256), 0, s,
                   grad, verts, bounds, ext, grid, proj, theta_e, lv, B, N, venc, Cout, qbuf, grad_verts);
        if (L > 0)
            VPN_LAUNCH(gcn_extent_bwd_kernel, dim3(B), dim3(256), 0, s, verts, ext, (const int*)ext_idx,
                       (const float*)qbuf, N, grad_verts);
    }
    VPN_LAUNCH_CHECK();
    return 0;
}
