// optim.hip — the optimiser stage (gfx950): Adam over every parameter of a group in ONE launch.
//
// Replaces (reference file:line) `Adam(params, lr, betas=(0.9, 0.99), weight_decay=W_DECAY)` (train.py:83-102,
// train_sphere.py:92, train_gcn.py:105), `optimizer.step()` (train.py:264, train_sphere.py:134, train_gcn.py:138) and, with
// zero_grads, the `optimizer.zero_grad()` before the next backward (train.py:262).  torch runs the step as a chain of
// multi-tensor passes over the same bytes with the step count in per-tensor state; here:
//   * a device table of segments {p, g, m, v, n, vec}, one row per parameter that has a gradient, and a device chunk table
//     (segment, first element), one row per workgroup of VPN_ADAM_CHUNK elements: a plain grid, no persistent loop, no grid
//     barrier (the house pattern of ragged_chunk_kernel, gtpoints.hip);
//   * a pure streaming kernel: 28 bytes per element (read p g m v, write p m v), 32 with gradient zeroing; 16-byte accesses
//     where the host found the four pointers of a segment 16-byte aligned (as fc_fwd_kernel's host side decides), element
//     accesses with the same indexing otherwise; no LDS, no scratch;
//   * a device state block {step, b1pow, b2pow, arrivals}: every workgroup reads it and forms the step's scalars in double;
//     the workgroup that arrives last (one arrival add behind a fence, the counter of loss_finalize_kernel in raster.hip,
//     without a payload to publish) advances it by one multiplication each.  A captured graph replays a fresh step
//     without the host.
// Compiled with -ffp-contract=off: every operation of vpn_hip.h's arithmetic is rounded by itself (tests/optim_ref.py
// restates it bit for bit), sqrt and divide are hipcc's IEEE defaults.
#include "vpn_common.h"

namespace vpn {

constexpr int AD_CHUNK = VPN_ADAM_CHUNK;
constexpr int AD_BLOCK = 256;
constexpr int AD_VEC = AD_CHUNK / (4 * AD_BLOCK);         // 16-byte accesses per lane and array in a full chunk
static_assert(AD_VEC * 4 * AD_BLOCK == AD_CHUNK && AD_BLOCK % 64 == 0, "a chunk is AD_VEC float4 for each of AD_BLOCK lanes");

struct AdamState { long long step; double b1pow, b2pow; unsigned arrivals, pad; };
static_assert(sizeof(AdamState) == VPN_ADAM_STATE_BYTES && sizeof(VpnAdamSegment) == 48, "the layouts of vpn_hip.h");

// The pointers of a segment come out of a table, so the compiler cannot know their address space and would use flat
// accesses: they are global memory by contract.  (Compiled as C++ for the host check the qualifier is empty.)
#if defined(__HIP_DEVICE_COMPILE__)
#define AD_GLOBAL __attribute__((address_space(1)))
typedef float V4 __attribute__((ext_vector_type(4)));
#else
#define AD_GLOBAL
typedef float4 V4;
#endif
typedef AD_GLOBAL float* GF;
typedef AD_GLOBAL V4* GV4;

struct AdamScalars { float c1, c2, b2f, wdf, epsf, bc2s, nss; bool decay; };

__device__ inline void adam_element(float& p, float g, float& m, float& v, const AdamScalars& k) {
#pragma clang fp contract(off)
    const float g1 = k.decay ? g + k.wdf * p : g;
    m = m + k.c1 * (g1 - m);
    v = v * k.b2f + k.c2 * (g1 * g1);
    const float den = sqrtf(v) / k.bc2s + k.epsf;
    p = p + k.nss * (m / den);
}

// four elements held as one 16-byte value (its components are no lvalues a reference could bind to)
__device__ inline void adam_four(V4& p, const V4& g, V4& m, V4& v, const AdamScalars& k) {
    float px = p.x, py = p.y, pz = p.z, pw = p.w, mx = m.x, my = m.y, mz = m.z, mw = m.w, vx = v.x, vy = v.y, vz = v.z, vw = v.w;
    adam_element(px, g.x, mx, vx, k); adam_element(py, g.y, my, vy, k);
    adam_element(pz, g.z, mz, vz, k); adam_element(pw, g.w, mw, vw, k);
    p.x = px; p.y = py; p.z = pz; p.w = pw; m.x = mx; m.y = my; m.z = mz; m.w = mw; v.x = vx; v.y = vy; v.z = vz; v.w = vw;
}

__device__ inline V4 zero_four() { V4 z; z.x = 0.0f; z.y = 0.0f; z.z = 0.0f; z.w = 0.0f; return z; }

__global__ __launch_bounds__(AD_BLOCK) void adam_step_kernel(const VpnAdamSegment* __restrict__ segments, int S,
                                                             const long long* __restrict__ chunks, int C, AdamState* state,
                                                             double lr, const float* __restrict__ lr_dev, double beta1,
                                                             double beta2, double eps, double wd, int zero_grads) {
    const int c = blockIdx.x, tid = threadIdx.x;
    // ---- the step's scalars, the same in every workgroup: the ADVANCED products, formed in double, rounded to fp32 once
    const long long step = state->step;
    const double B1 = state->b1pow * beta1, B2 = state->b2pow * beta2;
    if (lr_dev) lr = (double)lr_dev[0];
    AdamScalars k;
    k.c1 = (float)(1.0 - beta1); k.c2 = (float)(1.0 - beta2);
    k.b2f = (float)beta2; k.wdf = (float)wd; k.epsf = (float)eps;
    k.bc2s = (float)sqrt(1.0 - B2);
    k.nss = (float)(-(lr / (1.0 - B1)));
    k.decay = wd != 0.0;
    const bool zero = zero_grads != 0;

    // ---- this workgroup's chunk; the tables are data: clamped, so that a bad row can reach nothing outside its segment
    const long long seg_i = chunks[(size_t)c * 2], first = chunks[(size_t)c * 2 + 1];
    const VpnAdamSegment sg = segments[seg_i < 0 ? 0 : (seg_i >= S ? S - 1 : seg_i)];
    int cnt = 0;
    if (first >= 0 && first < sg.n) cnt = (int)(sg.n - first < AD_CHUNK ? sg.n - first : AD_CHUNK);
    const GF p = (GF)(sg.p + first), g = (GF)(sg.g + first), m = (GF)(sg.m + first), v = (GF)(sg.v + first);
    const GV4 p4 = (GV4)p, g4 = (GV4)g, m4 = (GV4)m, v4 = (GV4)v;
    const bool vec = sg.vec != 0 && (first & 3) == 0;      // float4 accesses need the chunk to start on one
    if (vec && cnt == AD_CHUNK) {
        // a full chunk: lane t owns the float4 t, t + 256, ...; all sixteen loads are issued before the first use
        V4 rp[AD_VEC], rg[AD_VEC], rm[AD_VEC], rv[AD_VEC];
#pragma unroll
        for (int j = 0; j < AD_VEC; ++j) {
            const int i = tid + j * AD_BLOCK;
            rp[j] = p4[i]; rg[j] = g4[i]; rm[j] = m4[i]; rv[j] = v4[i];
        }
#pragma unroll
        for (int j = 0; j < AD_VEC; ++j) {
            const int i = tid + j * AD_BLOCK;
            adam_four(rp[j], rg[j], rm[j], rv[j], k);
            p4[i] = rp[j]; m4[i] = rm[j]; v4[i] = rv[j];
            if (zero) g4[i] = zero_four();
        }
    } else {
        // a segment's last chunk, or a segment that is not 16-byte aligned: whole float4 where allowed, then elements
        const int n4 = vec ? cnt >> 2 : 0;
        for (int i = tid; i < n4; i += AD_BLOCK) {
            V4 pe = p4[i], me = m4[i], ve = v4[i];
            adam_four(pe, g4[i], me, ve, k);
            p4[i] = pe; m4[i] = me; v4[i] = ve;
            if (zero) g4[i] = zero_four();
        }
        for (int i = n4 * 4 + tid; i < cnt; i += AD_BLOCK) {
            float pe = p[i], me = m[i], ve = v[i];
            adam_element(pe, g[i], me, ve, k);
            p[i] = pe; m[i] = me; v[i] = ve;
            if (zero) g[i] = 0.0f;
        }
    }

    // ---- arrive; the last workgroup advances the state.  Every lane has used the state's values in its stores above, so
    // behind the barrier no wave of this workgroup reads the state again.  Nothing is handed to the last arriver but the
    // count itself (it advances the values IT read, and no workgroup has written the block in this launch), so the fence
    // in front of the add only keeps the compiler from moving the reads below it: workgroup scope.  An agent-scope release
    // here would write back the L2 once per chunk, thousands of times a launch, under the streaming stores.
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        const unsigned old = __hip_atomic_fetch_add(&state->arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (unsigned)C - 1u) {
            state->step = step + 1;
            state->b1pow = B1;
            state->b2pow = B2;
            __hip_atomic_store(&state->arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next step
        }
    }
}

static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace vpn

using namespace vpn;

extern "C" size_t vpn_adam_table_bytes(int segments, long long elements) {
    if (segments < 0 || elements < 0) return 0;
    return (size_t)segments * sizeof(VpnAdamSegment) + 16 * ((size_t)(elements / AD_CHUNK) + (size_t)segments);
}

extern "C" int vpn_adam_step(const VpnAdamSegment* segments, int num_segments, const long long* chunks, int num_chunks, void* state,
                             const double* hyper, const float* lr_dev, int zero_grads, void* stream) {
    if (num_segments < 0) return VPN_E_BADARG;
    if (num_segments == 0) return 0;                       // a group without gradients: nothing to do, the step does not advance
    if (!segments || !chunks || !state || !hyper) return VPN_E_BADARG;
    if (num_chunks <= 0) return VPN_E_BADARG;
    if (!aligned_to(segments, 8) || !aligned_to(chunks, 8) || !aligned_to(state, 8) || (lr_dev && !aligned_to(lr_dev, 4)))
        return VPN_E_BADARG;
    const double lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], wd = hyper[4];
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return VPN_E_BADARG;
    if (!(eps >= 0.0 && eps < INFINITY) || !(wd >= 0.0 && wd < INFINITY) || !(lr >= 0.0 && lr < INFINITY)) return VPN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(adam_step_kernel, dim3((unsigned)num_chunks), dim3(AD_BLOCK), 0, s, segments, num_segments, chunks, num_chunks,
               (AdamState*)state, lr, lr_dev, beta1, beta2, eps, wd, zero_grads);
    VPN_LAUNCH_CHECK();
    return 0;
}
