// gcnpair.hip — GCNModel's layer pairs as one linear map each.  conv_b(conv_a(x)) =
// A( A(x Theta_ab) + 1 (x) u ) + 1 (x) b_b with Theta_ab = Theta_a Theta_b and u = b_a Theta_b: one long product a pair, and
// the two aggregations back to back.
//
//   gcn_hop2_kernel          y = A( A h + u ) + b (+ ReLU) with both hops of a vertex block in LDS.  The block table
//                            (ops.gcn_blocks) cuts [0, N) into index ranges of at most GCN_HOP2_MAX_ROWS rows that no edge
//                            crosses, so a block's rows gather from that block alone: h is read once, y written once, the
//                            intermediate never reaches memory.  Every hop sums a row in CSR order with the multiply-add of
//                            gcn_aggregate_kernel (csrc/gcn.hip) and rounds the intermediate to fp32: y equals two launches
//                            of that kernel bit for bit.  The backward is the same kernel on the ReLU-masked gradient (A is
//                            symmetric); it also writes, per (sample, block, channel), the sum of its intermediate rows in
//                            row order, from which the gradient of u is a fixed-order column sum.
//   gcn_project_fwd_kernel   out [R, Co] = x [R, Ci] Theta [Ci, Co] for Co <= 4 (conv5 . conv6 has Co = 3): a wave per row,
//                            lanes across Ci, Theta in LDS, one butterfly a result.
//   gcn_project_bwd_kernel   dx = g Theta^T and the partial sums of dTheta = x^T g over 64-row chunks, one launch;
//   gcn_project_dtheta_kernel  the chunks added in order.  No atomics anywhere.
#include "vpn_common.h"

namespace vpn {

constexpr int GCN_HOP2_MAX_ROWS = 128;   // rows of a block (ops.GCN_HOP2_MAX_ROWS): the reference's 128-vertex spheres
// channels per workgroup: 2 x 128 x 16 floats of LDS = 16 KB.  A workgroup runs load, hop, hop in turn behind barriers, so
// the launch wants many of them a CU: at C = 512 (B 8, N 2048) forward 64 channels took 97 us, 32 took 63, 16 take 53
constexpr int GCN_HOP2_CH = 16;
constexpr int GCN_PROJECT_MAX_CO = 4;
constexpr int GCN_PROJECT_MAX_CI = 1024; // Theta [Ci, 4] in LDS: 16 KB (ops.GCN_PROJECT_MAX_CI)
constexpr int GCN_PROJECT_ROWS = 64;     // rows per workgroup of the backward, and per partial sum of dTheta
constexpr int GCN_PROJECT_FWD_ROWS = 16; // rows per workgroup of the forward: four a wave

// one hop of block rows [r0, r0 + rows) from LDS `src` ([row][cw]): element (r, q) = sum over row r0 + r's entries, in CSR
// order, with the multiply-add of gcn_aggregate_kernel
template <int V>
__device__ inline void gcn_hop2_row(const float* src, const int* __restrict__ row_ptr, const int* __restrict__ col,
                                    const float* __restrict__ w, int r0, int rows, int cw, int r, int q, float acc[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.0f;
    const int e1 = row_ptr[r0 + r + 1];
    for (int e = row_ptr[r0 + r]; e < e1; ++e) {
        const unsigned j = (unsigned)(col[e] - r0);
        const float a = w[e];
        if (j >= (unsigned)rows) continue;                 // an edge that leaves the block: the table forbids it
        const float* s = src + j * cw + q * V;
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(s);
            acc[0] = fmaf(a, v.x, acc[0]); acc[1] = fmaf(a, v.y, acc[1]);
            acc[2] = fmaf(a, v.z, acc[2]); acc[3] = fmaf(a, v.w, acc[3]);
        } else {
            acc[0] = fmaf(a, s[0], acc[0]);
        }
    }
}

// the (row, column) of a work-item's elements t, t + 256, ... of a block of nq columns, without a division per element
struct GcnHop2Walk {
    int r, q, rs, qs, nq;
    __device__ GcnHop2Walk(int t, int nq_) : nq(nq_) { r = t / nq; q = t - r * nq; rs = 256 / nq; qs = 256 - rs * nq; }
    __device__ void next() { r += rs; q += qs; if (q >= nq) { q -= nq; ++r; } }
};

// one workgroup per (block, 16-channel chunk, sample); V = 4: dwordx4 in memory and in LDS (C % 4 == 0)
template <int V>
__global__ __launch_bounds__(256) void gcn_hop2_kernel(const float* __restrict__ h, const float* __restrict__ mask,
                                                       const int* __restrict__ row_ptr, const int* __restrict__ col,
                                                       const float* __restrict__ w, const int* __restrict__ blocks,
                                                       const float* __restrict__ u, const float* __restrict__ bias, int N,
                                                       int C, int relu, int nblocks, float* __restrict__ out,
                                                       float* __restrict__ du_part) {
    __shared__ float s_h[GCN_HOP2_MAX_ROWS * GCN_HOP2_CH] __attribute__((aligned(16)));
    __shared__ float s_t[GCN_HOP2_MAX_ROWS * GCN_HOP2_CH] __attribute__((aligned(16)));
    const int blk = blockIdx.x, c0 = blockIdx.y * GCN_HOP2_CH, b = blockIdx.z, t = threadIdx.x;
    const int r0 = blocks[blk], r1 = blocks[blk + 1], rows = r1 - r0;
    if (r0 < 0 || rows <= 0 || rows > GCN_HOP2_MAX_ROWS || r1 > N) return;      // uniform: no table, no work
    const int cw = min(GCN_HOP2_CH, C - c0), nq = cw / V, items = rows * nq;
    const long long base = ((long long)b * N + r0) * C + c0;
    GcnHop2Walk at(t, nq);
    for (int i = t; i < items; i += 256, at.next()) {
        const long long src = base + (long long)at.r * C + at.q * V;
        if constexpr (V == 4) {
            float4 v = *reinterpret_cast<const float4*>(h + src);
            if (mask) {
                const float4 m = *reinterpret_cast<const float4*>(mask + src);
                v.x = m.x > 0.0f ? v.x : 0.0f; v.y = m.y > 0.0f ? v.y : 0.0f;
                v.z = m.z > 0.0f ? v.z : 0.0f; v.w = m.w > 0.0f ? v.w : 0.0f;
            }
            *reinterpret_cast<float4*>(&s_h[at.r * cw + at.q * 4]) = v;
        } else {
            float v = h[src];
            if (mask && !(mask[src] > 0.0f)) v = 0.0f;
            s_h[at.r * cw + at.q] = v;
        }
    }
    __syncthreads();
    at = GcnHop2Walk(t, nq);
    for (int i = t; i < items; i += 256, at.next()) {
        float acc[V];
        gcn_hop2_row<V>(s_h, row_ptr, col, w, r0, rows, cw, at.r, at.q, acc);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (u) acc[k] += u[c0 + at.q * V + k];
            s_t[at.r * cw + at.q * V + k] = acc[k];
        }
    }
    __syncthreads();
    if (du_part && t < cw) {                               // the intermediate's rows of this block, in row order
        float s = 0.0f;
        for (int r = 0; r < rows; ++r) s += s_t[r * cw + t];
        du_part[((long long)b * nblocks + blk) * C + c0 + t] = s;
    }
    at = GcnHop2Walk(t, nq);
    for (int i = t; i < items; i += 256, at.next()) {
        float acc[V];
        gcn_hop2_row<V>(s_t, row_ptr, col, w, r0, rows, cw, at.r, at.q, acc);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (bias) acc[k] += bias[c0 + at.q * V + k];
            if (relu) acc[k] = fmaxf(acc[k], 0.0f);
        }
        float* o = out + base + (long long)at.r * C + at.q * V;
        if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else o[0] = acc[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// out = x Theta, Co <= 4.  One workgroup per 16 rows (1024 workgroups at the reference's 16384 rows: the launch is bound by
// memory and wants every CU several times over), a wave per row and four rows of a wave in flight; lane l takes columns
// 4 l .. 4 l + 3 (+ 256 per pass; V = 1: l + 64 per pass), then the butterfly of wave_sum: the order is fixed.
template <int V>
__global__ __launch_bounds__(256) void gcn_project_fwd_kernel(const float* __restrict__ x, const float* __restrict__ theta,
                                                              int R, int Ci, int Co, float* __restrict__ out) {
    __shared__ float s_th[GCN_PROJECT_MAX_CI * 4] __attribute__((aligned(16)));
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    for (int i = t; i < Ci * 4; i += 256) {
        const int k = i >> 2, o = i & 3;
        s_th[i] = o < Co ? theta[(long long)k * Co + o] : 0.0f;
    }
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * GCN_PROJECT_FWD_ROWS;
    for (int rb = 0; rb < GCN_PROJECT_FWD_ROWS / 4; rb += 4) {
        float acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j][0] = 0.0f; acc[j][1] = 0.0f; acc[j][2] = 0.0f; acc[j][3] = 0.0f; }
        for (int k = lane * V; k < Ci; k += 64 * V) {
            float xv[4][V];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long row = row0 + wv + 4 * (rb + j);
                if constexpr (V == 4) {
                    const float4 q = row < R ? *reinterpret_cast<const float4*>(x + row * Ci + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    xv[j][0] = q.x; xv[j][1] = q.y; xv[j][2] = q.z; xv[j][3] = q.w;
                } else {
                    xv[j][0] = row < R ? x[row * Ci + k] : 0.0f;
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float4 th = *reinterpret_cast<const float4*>(&s_th[(k + i) * 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j][0] = fmaf(xv[j][i], th.x, acc[j][0]); acc[j][1] = fmaf(xv[j][i], th.y, acc[j][1]);
                    acc[j][2] = fmaf(xv[j][i], th.z, acc[j][2]); acc[j][3] = fmaf(xv[j][i], th.w, acc[j][3]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s0 = wave_sum(acc[j][0]), s1 = wave_sum(acc[j][1]), s2 = wave_sum(acc[j][2]), s3 = wave_sum(acc[j][3]);
            const long long row = row0 + wv + 4 * (rb + j);
            if (row < R && lane < Co) out[row * Co + lane] = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : s3;
        }
    }
}

// dx = g Theta^T and ws [P, Ci, Co] = the sums of x^T g over 64-row chunks.  One workgroup per (chunk, 64 V columns): lane l
// owns V columns of x and dx with their rows of Theta in registers, wave w takes rows w, w + 4, ... of the chunk, and the
// four waves' sums are added in a fixed order through LDS.  dx == NULL / ws == NULL: that half is skipped.
template <int V>
__global__ __launch_bounds__(256) void gcn_project_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                              const float* __restrict__ theta, int R, int Ci, int Co,
                                                              float* __restrict__ dx, float* __restrict__ ws) {
    __shared__ float s_g[GCN_PROJECT_ROWS * 4] __attribute__((aligned(16)));
    __shared__ float s_part[3 * 4 * V * 64];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, p = blockIdx.x;
    const long long r0 = (long long)p * GCN_PROJECT_ROWS;
    const int nr = (int)(R - r0 < GCN_PROJECT_ROWS ? R - r0 : GCN_PROJECT_ROWS);
    {
        const int r = t >> 2, o = t & 3;
        s_g[t] = (r < nr && o < Co) ? g[(r0 + r) * Co + o] : 0.0f;
    }
    __syncthreads();
    const int k = (blockIdx.y * 64 + lane) * V;
    const bool live = k < Ci;                               // V = 4: Ci % 4 == 0, so k + 3 is a column when k is
    float th[V][4], acc[V][4];
#pragma unroll
    for (int i = 0; i < V; ++i) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            th[i][o] = (live && dx && o < Co) ? theta[(long long)(k + i) * Co + o] : 0.0f;
            acc[i][o] = 0.0f;
        }
    }
#pragma unroll 4
    for (int r = wv; r < nr; r += 4) {
        const float4 gv = *reinterpret_cast<const float4*>(&s_g[r * 4]);
        if (!live) continue;
        const long long at = (r0 + r) * Ci + k;
        if (ws) {
            float xv[V];
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4*>(x + at);
                xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
            } else {
                xv[0] = x[at];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                acc[i][0] = fmaf(xv[i], gv.x, acc[i][0]); acc[i][1] = fmaf(xv[i], gv.y, acc[i][1]);
                acc[i][2] = fmaf(xv[i], gv.z, acc[i][2]); acc[i][3] = fmaf(xv[i], gv.w, acc[i][3]);
            }
        }
        if (dx) {
            float d[V];
#pragma unroll
            for (int i = 0; i < V; ++i)
                d[i] = fmaf(gv.w, th[i][3], fmaf(gv.z, th[i][2], fmaf(gv.y, th[i][1], gv.x * th[i][0])));
            if constexpr (V == 4) *reinterpret_cast<float4*>(dx + at) = make_float4(d[0], d[1], d[2], d[3]);
            else dx[at] = d[0];
        }
    }
    if (!ws) return;                                        // uniform
    if (wv > 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
#pragma unroll
            for (int o = 0; o < 4; ++o) s_part[((wv - 1) * 4 * V + i * 4 + o) * 64 + lane] = acc[i][o];
        }
    }
    __syncthreads();
    if (wv == 0 && live) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (o < Co)
                    ws[((long long)p * Ci + k + i) * Co + o] =
                        ((acc[i][o] + s_part[(0 * 4 * V + i * 4 + o) * 64 + lane]) + s_part[(1 * 4 * V + i * 4 + o) * 64 + lane]) +
                        s_part[(2 * 4 * V + i * 4 + o) * 64 + lane];
        }
    }
}

__global__ __launch_bounds__(256) void gcn_project_dtheta_kernel(const float* __restrict__ ws, int n, int P,
                                                                 float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int p = 0; p < P; ++p) acc += ws[(long long)p * n + i];
    out[i] = acc;
}

}  // namespace vpn

using namespace vpn;

static bool gcnpair_aligned(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" size_t vpn_gcn_aggregate2_workspace(int B, int nblocks, int C) {
    if (B <= 0 || nblocks <= 0 || C <= 0) return 0;
    return (size_t)B * nblocks * C * sizeof(float);
}

extern "C" int vpn_gcn_aggregate2(const float* h, const float* mask, const int32_t* row_ptr, const int32_t* col,
                                  const float* w, const int32_t* blocks, int nblocks, const float* u, const float* bias,
                                  int B, int N, int C, int relu, float* out, float* du_partial, void* stream) {
    if (!h || !row_ptr || !col || !w || !blocks || !out || B <= 0 || N <= 0 || C <= 0 || nblocks <= 0 || nblocks > N)
        return VPN_E_BADARG;
    if ((long long)B * N * C > 0x7fffffffLL * 4) return VPN_E_TOOBIG;
    const int chunks = (C + GCN_HOP2_CH - 1) / GCN_HOP2_CH;
    if (chunks > 65535 || B > 65535) return VPN_E_TOOBIG;
    const bool v4 = (C % 4) == 0 && gcnpair_aligned(h) && gcnpair_aligned(out) && gcnpair_aligned(mask);
    const dim3 grid(nblocks, chunks, B);
    if (v4)
        VPN_LAUNCH_AS("gcn_hop2_kernel", gcn_hop2_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, h, mask,
                      (const int*)row_ptr, (const int*)col, w, (const int*)blocks, u, bias, N, C, relu, nblocks, out,
                      du_partial);
    else
        VPN_LAUNCH_AS("gcn_hop2_kernel", gcn_hop2_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, h, mask,
                      (const int*)row_ptr, (const int*)col, w, (const int*)blocks, u, bias, N, C, relu, nblocks, out,
                      du_partial);
    VPN_LAUNCH_CHECK();
    return 0;
}

static int gcn_project_check(int R, int Ci, int Co) {
    if (R <= 0 || Ci <= 0 || Co <= 0 || Co > GCN_PROJECT_MAX_CO || Ci > GCN_PROJECT_MAX_CI) return VPN_E_BADARG;
    if ((long long)R * Ci > 0x7fffffffLL * 4) return VPN_E_TOOBIG;
    return 0;
}

extern "C" size_t vpn_gcn_project_bwd_workspace(int R, int Ci, int Co) {
    if (gcn_project_check(R, Ci, Co)) return 0;
    return (size_t)((R + GCN_PROJECT_ROWS - 1) / GCN_PROJECT_ROWS) * Ci * Co * sizeof(float);
}

extern "C" int vpn_gcn_project_fwd(const float* x, const float* theta, int R, int Ci, int Co, float* out, void* stream) {
    if (!x || !theta || !out) return VPN_E_BADARG;
    const int rc = gcn_project_check(R, Ci, Co);
    if (rc) return rc;
    const dim3 grid((unsigned)((R + GCN_PROJECT_FWD_ROWS - 1) / GCN_PROJECT_FWD_ROWS));
    if ((Ci % 4) == 0 && gcnpair_aligned(x))
        VPN_LAUNCH_AS("gcn_project_fwd_kernel", gcn_project_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, theta,
                      R, Ci, Co, out);
    else
        VPN_LAUNCH_AS("gcn_project_fwd_kernel", gcn_project_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, theta,
                      R, Ci, Co, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_gcn_project_bwd(const float* grad, const float* x, const float* theta, int R, int Ci, int Co,
                                   void* workspace, float* dx, float* dtheta, void* stream) {
    if (!grad) return VPN_E_BADARG;
    const int rc = gcn_project_check(R, Ci, Co);
    if (rc) return rc;
    if (!dx && !dtheta) return 0;
    if ((dx && !theta) || (dtheta && (!x || !workspace))) return VPN_E_BADARG;
    const int P = (R + GCN_PROJECT_ROWS - 1) / GCN_PROJECT_ROWS;
    float* ws = dtheta ? (float*)workspace : nullptr;
    const bool v4 = (Ci % 4) == 0 && gcnpair_aligned(x) && gcnpair_aligned(dx);
    const int per = 64 * (v4 ? 4 : 1);
    const dim3 grid(P, (Ci + per - 1) / per);
    if (v4)
        VPN_LAUNCH_AS("gcn_project_bwd_kernel", gcn_project_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, grad, x,
                      theta, R, Ci, Co, dx, ws);
    else
        VPN_LAUNCH_AS("gcn_project_bwd_kernel", gcn_project_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, grad, x,
                      theta, R, Ci, Co, dx, ws);
    if (dtheta)
        VPN_LAUNCH(gcn_project_dtheta_kernel, dim3((Ci * Co + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                   (const float*)ws, Ci * Co, P, dtheta);
    VPN_LAUNCH_CHECK();
    return 0;
}
