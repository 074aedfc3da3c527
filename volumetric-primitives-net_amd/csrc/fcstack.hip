// fcstack.hip — the FC heads of the networks: G groups of L nn.Linear layers with nothing between them but an optional
// dropout, forward and backward, one launch per layer covering every group.
//
// Replaces volume_fc / rotate_fc / translate_fc of the reference's models (modules/network/vpnet_one_resnet.py:31-33,
// :87-107; vpnet_two_resnet.py:34-36, :90-110) and SDNet's deform stack (sdnet.py:19, :41-50), together with what follows
// the last layer: nothing, SDNet's tanh (sdnet.py:48), or restrict_range + split + restrict_volumes
// (vpnet_one_resnet.py:34-41, :67-85) written straight into the packed [B,K,10] rows (the rule of vpn_head_rule.h).
//
// The stage is weight traffic: at B <= 64 a layer is a skinny GEMM whose arithmetic is negligible next to the 4 MB of
// fp32 weights it streams.  So every kernel is organised around reading a weight ONCE, coalesced, into registers:
//   fc_fwd_kernel     a wave owns 4 weight rows (64 registers at in <= 1024) and runs every batch row past them; the
//                     input rows of the workgroup come through LDS, 8 at a time; wave_sum finishes each dot product
//   fc_bwd_kernel     two roles in one launch: workgroups [0, nxb) form dX partial sums (a wave owns 256 input columns
//                     and 32 weight rows, held in 128 registers while it walks the batch 16 rows at a time; lanes
//                     never exchange anything) and the others form dW = dY^T X and db from the activations alone
//                     (a thread owns 4 x 4 weights, the batch is walked in order)
//   fc_reduce_kernel  adds the dX partial sums of the ceil(out / 32) row slices in slice order, applies the dropout mask
//                     of the layer below and writes that layer's dY (or the input gradient)
// No float atomics and no grid-wide barrier: every sum has one fixed order, so outputs and gradients are bit-equal from
// run to run.  Nothing synchronises with the host; nothing is allocated.
#include "vpn_head_rule.h"

namespace vpn {

constexpr int FC_ROWS = 4;        // weight rows of a wave (forward)
constexpr int FC_BR = 16;         // ... of a workgroup: 4 waves
constexpr int FC_KT = 1024;       // input columns held in registers at a time: 4 float4 per lane and row
constexpr int FC_BC = 8;          // batch rows staged in LDS at a time (forward): 32 KB
constexpr int FC_XC = 256;        // input columns of a dX wave: one float4 per lane
constexpr int FC_XB = 8;          // batch rows a dX wave takes at a time: 8 float4 accumulators beside its 32 of weights
constexpr int FC_OS = VPN_FC_SLICE;   // weight rows of a dX slice
constexpr int FC_WC = 1024;       // input columns of a dW workgroup: one float4 per thread
constexpr int FC_WB = 64;         // batch rows whose dY a dW workgroup stages at a time

struct FcRun {
    int layer, vec, dropout, epilogue, K;
    float p;
    uint64_t seed;
    const uint64_t* seed_dev;      // NULL, or a device word added to seed (a step counter: graph replays draw anew)
    HeadRule h;
    float* final;
};

struct FcBwdRun {
    int layer, vec, dropout, epilogue, K, nxb;
    float p;
    uint64_t seed;
    const uint64_t* seed_dev;
    HeadRule h;
    float* part;        // [G][slice][B][in] partial dX
    float* dy;          // [G][B][width]: dY of the layer the launch works on
    size_t part_stride, dy_stride;      // floats per group
};

__device__ inline float4 fc_ld4(const float* p, int col, int n, int vec) {       // p[col .. col+3], zero beyond n
    if (vec) return col < n ? *reinterpret_cast<const float4*>(p + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v;
    v.x = col < n ? p[col] : 0.f;
    v.y = col + 1 < n ? p[col + 1] : 0.f;
    v.z = col + 2 < n ? p[col + 2] : 0.f;
    v.w = col + 3 < n ? p[col + 3] : 0.f;
    return v;
}

__device__ inline void fc_st4(float* p, int col, int n, int vec, float4 v) {
    if (vec) { if (col < n) *reinterpret_cast<float4*>(p + col) = v; return; }
    if (col < n) p[col] = v.x;
    if (col + 1 < n) p[col + 1] = v.y;
    if (col + 2 < n) p[col + 2] = v.z;
    if (col + 3 < n) p[col + 3] = v.w;
}

// keep decision of output o of batch row b after layer l of group g: the caller's mask, or Philox keyed by all five
__device__ inline bool fc_keep(const uint8_t* mask, int dropout, float p, uint64_t seed, int g, int l, int b, int o, int out) {
    if (dropout == VPN_FC_DROPOUT_MASK) return mask[(size_t)b * out + o] != 0;
    uint32_t r[4];
    philox4x32_10((uint32_t)o, (uint32_t)b, (uint32_t)l, (uint32_t)g, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return (float)(r[0] >> 8) * 5.9604644775390625e-08f >= p;
}

// where output o of group g lands in a packed row: volumes | rotates | translates (split(3|4|3), :36-38)
__device__ inline void fc_pack_slot(int g, int o, int& k, int& f) {
    const int w = g == 1 ? 4 : 3, f0 = g == 0 ? 0 : (g == 1 ? 3 : 7);
    k = o / w;
    f = f0 + (o - k * w);
}

__global__ __launch_bounds__(256) void fc_fwd_kernel(const VpnFcStack s, const FcRun a) {
    __shared__ float4 xs[FC_BC][FC_KT / 4];
    const int g = blockIdx.y, l = a.layer, L = s.L, B = s.B;
    const int in = l == 0 ? s.in0[g] : s.out[g * L + l - 1], out = s.out[g * L + l];
    if ((int)blockIdx.x * FC_BR >= out) return;                      // the whole workgroup: no barrier is left behind
    const float* x = l == 0 ? s.x[g] : s.act[g * L + l - 1];
    const float* W = s.w[g * L + l];
    const float* bias = s.bias[g * L + l];
    float* y = s.act[g * L + l];
    const int tx = threadIdx.x, wave = tx >> 6, lane = tx & 63;
    const int row0 = blockIdx.x * FC_BR + wave * FC_ROWS;
    const int ntiles = (in + FC_KT - 1) / FC_KT;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * FC_KT;
        float4 w[FC_ROWS][4];
#pragma unroll
        for (int r = 0; r < FC_ROWS; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = row0 + r;
                w[r][q] = o < out ? fc_ld4(W + (size_t)o * in, k0 + (q * 64 + lane) * 4, in, a.vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        for (int b0 = 0; b0 < B; b0 += FC_BC) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < FC_BC; ++i)
                xs[i][tx] = b0 + i < B ? fc_ld4(x + (size_t)(b0 + i) * in, k0 + tx * 4, in, a.vec) : make_float4(0.f, 0.f, 0.f, 0.f);
            __syncthreads();
            float mine = 0.f;                                        // lane bl * FC_ROWS + r keeps the dot product (bl, r)
#pragma unroll
            for (int bl = 0; bl < FC_BC; ++bl) {
                float pr[FC_ROWS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 xv = xs[bl][q * 64 + lane];
#pragma unroll
                    for (int r = 0; r < FC_ROWS; ++r)
                        pr[r] += w[r][q].x * xv.x + w[r][q].y * xv.y + w[r][q].z * xv.z + w[r][q].w * xv.w;
                }
#pragma unroll
                for (int r = 0; r < FC_ROWS; ++r) {
                    const float sum = wave_sum(pr[r]);
                    if (lane == bl * FC_ROWS + r) mine = sum;
                }
            }
            const int b = b0 + lane / FC_ROWS, o = row0 + lane % FC_ROWS;
            if (lane < FC_BC * FC_ROWS && b < B && o < out) {
                const size_t idx = (size_t)b * out + o;
                float v = (t == 0 ? bias[o] : y[idx]) + mine;        // a later tile adds to what this lane wrote itself
                if (t == ntiles - 1) {
                    if (l < L - 1) {
                        if (a.dropout) v = fc_keep(s.keep[g * L + l], a.dropout, a.p, a.seed + (a.seed_dev ? *a.seed_dev : 0), g, l, b, o, out) ? v * (1.0f / (1.0f - a.p)) : 0.0f;
                    } else if (a.epilogue == VPN_FC_TANH) {
                        a.final[idx] = tanhf(v);                     // sdnet.py:48
                    } else if (a.epilogue == VPN_FC_VP_PACK) {
                        int k, f;
                        float yv, dy;
                        fc_pack_slot(g, o, k, f);
                        head_field(a.h, f, v, yv, dy);
                        a.final[((size_t)b * a.K + k) * VPN_PARAM_STRIDE + f] = yv;
                    }
                }
                y[idx] = v;                                          // last layer: the raw output, kept for the backward
            }
        }
    }
}

// dL/d(raw output o of batch row b) of the layer the launch works on
__device__ inline float fc_dy(const VpnFcStack& s, const VpnFcGrad& gr, const FcBwdRun& a, int g, int b, int o, int out) {
    const int L = s.L;
    const size_t idx = (size_t)b * out + o;
    if (a.layer < L - 1) return a.dy[g * a.dy_stride + idx];
    if (a.epilogue == VPN_FC_NONE) return gr.gout[g][idx];
    const float raw = s.act[g * L + L - 1][idx];
    if (a.epilogue == VPN_FC_TANH) { const float t = tanhf(raw); return gr.gout[0][idx] * (1.0f - t * t); }
    int k, f;
    float yv, dy;
    fc_pack_slot(g, o, k, f);
    head_field(a.h, f, raw, yv, dy);
    return gr.gout[0][((size_t)b * a.K + k) * VPN_PARAM_STRIDE + f] * dy;
}

__global__ __launch_bounds__(256) void fc_bwd_kernel(const VpnFcStack s, const VpnFcGrad gr, const FcBwdRun a) {
    __shared__ float4 dys[4][FC_OS][FC_XB / 4];      // dX role: per wave, the dY of its slice and batch rows
    __shared__ float4 dyw[FC_WB];                    // dW role: dY of 4 rows, FC_WB batch rows
    const int g = blockIdx.y, l = a.layer, L = s.L, B = s.B;
    const int in = l == 0 ? s.in0[g] : s.out[g * L + l - 1], out = s.out[g * L + l];
    const float* x = l == 0 ? s.x[g] : s.act[g * L + l - 1];
    const int tx = threadIdx.x, wave = tx >> 6, lane = tx & 63;
    if ((int)blockIdx.x < a.nxb) {
        // ---- dX partial sums: part[g][slice][b][i] = sum over the slice's rows o of dY[b,o] W[o,i]
        if (l == 0 && !gr.dx[g]) return;
        const float* W = s.w[g * L + l];
        const int tiles = (in + FC_XC - 1) / FC_XC, S = (out + FC_OS - 1) / FC_OS, nbc = (B + FC_XB - 1) / FC_XB;
        const int j = blockIdx.x * 4 + wave;
        const bool live = j < tiles * S;
        const int tile = j % tiles, sl = j / tiles;
        const int col = tile * FC_XC + lane * 4;
        const int rows = live ? min(FC_OS, out - sl * FC_OS) : 0;
        float4 wv[FC_OS];                               // the wave's weights, read once, kept for every batch chunk
#pragma unroll
        for (int ol = 0; ol < FC_OS; ++ol)
            wv[ol] = ol < rows ? fc_ld4(W + (size_t)(sl * FC_OS + ol) * in, col, in, a.vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        float* d = reinterpret_cast<float*>(&dys[wave][0][0]);
        float* part = a.part + g * a.part_stride;
        for (int bc = 0; bc < nbc; ++bc) {              // nbc is the same for every wave of the launch: the barriers match
            __syncthreads();
            for (int e = lane; e < FC_OS * FC_XB; e += 64) {
                const int ol = e / FC_XB, b = bc * FC_XB + e % FC_XB;
                d[e] = (ol < rows && b < B) ? fc_dy(s, gr, a, g, b, sl * FC_OS + ol, out) : 0.0f;
            }
            __syncthreads();
            float4 acc[FC_XB];
#pragma unroll
            for (int bl = 0; bl < FC_XB; ++bl) acc[bl] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int ol = 0; ol < FC_OS; ++ol) {
#pragma unroll
                for (int q = 0; q < FC_XB / 4; ++q) {
                    const float4 dv = dys[wave][ol][q];
                    const float dd[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        acc[4 * q + t].x += dd[t] * wv[ol].x; acc[4 * q + t].y += dd[t] * wv[ol].y;
                        acc[4 * q + t].z += dd[t] * wv[ol].z; acc[4 * q + t].w += dd[t] * wv[ol].w;
                    }
                }
            }
            if (live) {
#pragma unroll
                for (int bl = 0; bl < FC_XB; ++bl) {
                    const int b = bc * FC_XB + bl;
                    if (b < B) fc_st4(part + ((size_t)sl * B + b) * in, col, in, a.vec, acc[bl]);
                }
            }
        }
        return;
    }
    // ---- dW[o,i] = sum_b dY[b,o] X[b,i], db[o] = sum_b dY[b,o], b in order; skipped for a frozen group
    float* dW = gr.dw[g * L + l];
    float* db = gr.db[g * L + l];
    if (!dW && !db) return;
    const int wb = blockIdx.x - a.nxb, tiles = (in + FC_WC - 1) / FC_WC;
    const int tile = wb % tiles, row0 = (wb / tiles) * 4;
    if (row0 >= out) return;
    const int col = tile * FC_WC + tx * 4;
    float4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    float bsum = 0.f;
    float* dl = reinterpret_cast<float*>(dyw);
    for (int b0 = 0; b0 < B; b0 += FC_WB) {
        __syncthreads();
        {
            const int b = b0 + tx / 4, o = row0 + tx % 4;
            dl[tx] = (b < B && o < out) ? fc_dy(s, gr, a, g, b, o, out) : 0.0f;
        }
        __syncthreads();
        const int nb = min(FC_WB, B - b0);
        for (int bl = 0; bl < nb; ++bl) {
            const float4 xv = fc_ld4(x + (size_t)(b0 + bl) * in, col, in, a.vec);
            const float4 dv = dyw[bl];
            acc[0].x += dv.x * xv.x; acc[0].y += dv.x * xv.y; acc[0].z += dv.x * xv.z; acc[0].w += dv.x * xv.w;
            acc[1].x += dv.y * xv.x; acc[1].y += dv.y * xv.y; acc[1].z += dv.y * xv.z; acc[1].w += dv.y * xv.w;
            acc[2].x += dv.z * xv.x; acc[2].y += dv.z * xv.y; acc[2].z += dv.z * xv.z; acc[2].w += dv.z * xv.w;
            acc[3].x += dv.w * xv.x; acc[3].y += dv.w * xv.y; acc[3].z += dv.w * xv.z; acc[3].w += dv.w * xv.w;
        }
        if (tile == 0 && tx < 4)
            for (int bl = 0; bl < nb; ++bl) bsum += dl[bl * 4 + tx];
    }
    if (dW) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row0 + r < out) fc_st4(dW + (size_t)(row0 + r) * in, col, in, a.vec, acc[r]);
    }
    if (db && tile == 0 && tx < 4 && row0 + tx < out) db[row0 + tx] = bsum;
}

// dX[b,i] = the slices' partial sums in slice order; times the dropout mask of layer l-1; becomes that layer's dY
__global__ __launch_bounds__(256) void fc_reduce_kernel(const VpnFcStack s, const VpnFcGrad gr, const FcBwdRun a) {
    const int g = blockIdx.y, l = a.layer, L = s.L, B = s.B;
    const int in = l == 0 ? s.in0[g] : s.out[g * L + l - 1], out = s.out[g * L + l];
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)B * in) return;
    if (l == 0 && !gr.dx[g]) return;
    const int S = (out + FC_OS - 1) / FC_OS;
    const float* part = a.part + g * a.part_stride + e;
    float v = 0.f;
    for (int sl = 0; sl < S; ++sl) v += part[(size_t)sl * B * in];
    if (l == 0) { gr.dx[g][e] = v; return; }
    if (a.dropout) {
        const int b = (int)(e / in), i = (int)(e - (long long)b * in);
        v = fc_keep(s.keep[g * L + l - 1], a.dropout, a.p, a.seed + (a.seed_dev ? *a.seed_dev : 0), g, l - 1, b, i, in) ? v * (1.0f / (1.0f - a.p)) : 0.0f;
    }
    a.dy[g * a.dy_stride + e] = v;
}

}  // namespace vpn

using namespace vpn;

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// everything a launch relies on, checked on the host before anything touches the GPU; *maxw: the widest layer side
static int fc_check(const VpnFcStack& s, int dropout, float p, int epilogue, int K, float r0, float r1, float r2,
                    const float* final, int* maxw) {
    if (s.G <= 0 || s.L <= 0 || s.B <= 0) return VPN_E_BADARG;
    if (s.L > VPN_FC_MAX_LAYERS || (long long)s.G * s.L > VPN_FC_MAX_SLOTS) return VPN_E_TOOBIG;
    if (dropout < VPN_FC_DROPOUT_OFF || dropout > VPN_FC_DROPOUT_PHILOX) return VPN_E_BADARG;
    if (dropout && !(p >= 0.0f && p < 1.0f)) return VPN_E_BADARG;
    if (epilogue < VPN_FC_NONE || epilogue > VPN_FC_VP_PACK) return VPN_E_BADARG;
    int m = 0;
    for (int g = 0; g < s.G; ++g) {
        if (!s.x[g] || s.in0[g] <= 0) return VPN_E_BADARG;
        m = s.in0[g] > m ? s.in0[g] : m;
        for (int l = 0; l < s.L; ++l) {
            const int i = g * s.L + l;
            if (!s.w[i] || !s.bias[i] || !s.act[i] || s.out[i] <= 0) return VPN_E_BADARG;
            if (dropout == VPN_FC_DROPOUT_MASK && l < s.L - 1 && !s.keep[i]) return VPN_E_BADARG;
            m = s.out[i] > m ? s.out[i] : m;
        }
    }
    if ((long long)s.B * m > 0x7fffffffLL / 4) return VPN_E_TOOBIG;
    if (epilogue != VPN_FC_NONE && !final) return VPN_E_BADARG;
    if (epilogue == VPN_FC_TANH && s.G != 1) return VPN_E_BADARG;
    if (epilogue == VPN_FC_VP_PACK) {
        if (s.G != 3 || K <= 0) return VPN_E_BADARG;
        if (!(r0 > 0.0f) || !(r1 > 0.0f) || !(r2 > 0.0f)) return VPN_E_BADARG;
        const int L = s.L;
        if (s.out[L - 1] != 3 * K || s.out[2 * L - 1] != 4 * K || s.out[3 * L - 1] != 3 * K) return VPN_E_BADARG;
    }
    *maxw = m;
    return 0;
}

static int fc_in(const VpnFcStack& s, int g, int l) { return l == 0 ? s.in0[g] : s.out[g * s.L + l - 1]; }
static const float* fc_x(const VpnFcStack& s, int g, int l) { return l == 0 ? s.x[g] : s.act[g * s.L + l - 1]; }

extern "C" size_t vpn_fc_stack_workspace(int G, int B, int max_width) {
    if (G <= 0 || B <= 0 || max_width <= 0) return 0;
    const size_t w4 = ((size_t)max_width + 3) / 4 * 4, S = ((size_t)max_width + FC_OS - 1) / FC_OS;
    return (size_t)G * B * w4 * (S + 1) * sizeof(float);
}

extern "C" int vpn_fc_stack_fwd(VpnFcStack s, int dropout, float p, uint64_t seed, const uint64_t* seed_dev, int epilogue, int K, int is_sigmoid,
                                float clamp_min, float clamp_max, float restrict0, float restrict1, float restrict2,
                                float* final, void* stream) {
    int maxw = 0;
    int rc = fc_check(s, dropout, p, epilogue, K, restrict0, restrict1, restrict2, final, &maxw);
    if (rc) return rc;
    FcRun a;
    a.dropout = dropout; a.epilogue = epilogue; a.K = K; a.p = p; a.seed = seed; a.seed_dev = seed_dev; a.final = final;
    a.h = HeadRule{is_sigmoid, clamp_min, clamp_max, restrict0, restrict1, restrict2};
    for (int l = 0; l < s.L; ++l) {
        int vec = 1, mo = 0;
        for (int g = 0; g < s.G; ++g) {
            vec &= fc_in(s, g, l) % 4 == 0 && al16(s.w[g * s.L + l]) && al16(fc_x(s, g, l));
            mo = s.out[g * s.L + l] > mo ? s.out[g * s.L + l] : mo;
        }
        a.layer = l; a.vec = vec;
        VPN_LAUNCH(fc_fwd_kernel, dim3((mo + FC_BR - 1) / FC_BR, s.G), dim3(256), 0, (hipStream_t)stream, s, a);
        VPN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int vpn_fc_stack_bwd(VpnFcStack s, VpnFcGrad gr, int dropout, float p, uint64_t seed, const uint64_t* seed_dev,
                                int epilogue, int K,
                                int is_sigmoid, float clamp_min, float clamp_max, float restrict0, float restrict1,
                                float restrict2, void* workspace, size_t workspace_bytes, void* stream) {
    int maxw = 0;
    // the forward's `final` is not read here: any non-null stand-in satisfies the shared check
    int rc = fc_check(s, dropout, p, epilogue, K, restrict0, restrict1, restrict2, (const float*)workspace, &maxw);
    if (rc) return rc;
    if (!workspace || !al16(workspace)) return VPN_E_BADARG;
    if (workspace_bytes < vpn_fc_stack_workspace(s.G, s.B, maxw)) return VPN_E_BADARG;
    for (int g = 0; g < (epilogue == VPN_FC_NONE ? s.G : 1); ++g)
        if (!gr.gout[g]) return VPN_E_BADARG;
    const size_t w4 = ((size_t)maxw + 3) / 4 * 4, S = ((size_t)maxw + FC_OS - 1) / FC_OS;
    FcBwdRun a;
    a.dropout = dropout; a.epilogue = epilogue; a.K = K; a.p = p; a.seed = seed; a.seed_dev = seed_dev;
    a.h = HeadRule{is_sigmoid, clamp_min, clamp_max, restrict0, restrict1, restrict2};
    a.part = (float*)workspace;
    a.part_stride = S * s.B * w4;
    a.dy = a.part + (size_t)s.G * a.part_stride;
    a.dy_stride = (size_t)s.B * w4;
    for (int l = s.L - 1; l >= 0; --l) {
        int vec = 1, any_dx = l > 0, any_dw = 0;
        long long nx = 0, nw = 0, ne = 0;
        for (int g = 0; g < s.G; ++g) {
            const int in = fc_in(s, g, l), out = s.out[g * s.L + l], i = g * s.L + l;
            vec &= in % 4 == 0 && al16(s.w[i]) && al16(fc_x(s, g, l)) && (!gr.dw[i] || al16(gr.dw[i]));
            if (l == 0 && gr.dx[g]) any_dx = 1;
            if (gr.dw[i] || gr.db[i]) any_dw = 1;
            const long long jx = (long long)((in + FC_XC - 1) / FC_XC) * ((out + FC_OS - 1) / FC_OS);
            const long long jw = (long long)((in + FC_WC - 1) / FC_WC) * ((out + 3) / 4);
            nx = jx > nx ? jx : nx;
            nw = jw > nw ? jw : nw;
            ne = (long long)s.B * in > ne ? (long long)s.B * in : ne;
        }
        a.layer = l; a.vec = vec;
        a.nxb = any_dx ? (int)((nx + 3) / 4) : 0;
        const long long blocks = a.nxb + (any_dw ? nw : 0);
        if (blocks > 0x7fffffffLL) return VPN_E_TOOBIG;
        if (blocks > 0) {
            VPN_LAUNCH(fc_bwd_kernel, dim3((unsigned)blocks, s.G), dim3(256), 0, (hipStream_t)stream, s, gr, a);
            VPN_LAUNCH_CHECK();
        }
        if (any_dx) {
            VPN_LAUNCH(fc_reduce_kernel, dim3((unsigned)((ne + 255) / 256), s.G), dim3(256), 0, (hipStream_t)stream, s, gr, a);
            VPN_LAUNCH_CHECK();
        }
    }
    return 0;
}
