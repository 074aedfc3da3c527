// evaluate.hip — the evaluation stage (test.py:68-135, test_gcn.py:115-178): per-sample Chamfer and EMD metrics of a
// batch and the per-class bookkeeping of an evaluation epoch, on the device.  One launch per batch replaces the final
// reduction of ChamferDistanceLoss(each_batch=True), torch.sqrt(dist).mean(1), the two batch means and the
// `for b in range(B)` loop with its 2 + 2 B .item() calls (test_gcn.py:145-152).
//
// State (include/vpn_hip.h, vpn_eval_state_size): 3 + 2 C doubles, then 2 + C int64, zeroed by the caller:
//   d[0] total_cd   d[1] total_emd   d[2] the arrival ticket of the launch in flight (an int in an 8-byte slot; 0 between
//   launches, so it reads as 0.0)   d[3 .. 3+C) class_sum_cd   d[3+C .. 3+2C) class_sum_emd
//   n[0] n_batches  n[1] n_invalid  n[2 .. 2+C) class_n
//
// Built with -ffp-contract=off: cd_b must be the bits of vpn_chamfer_loss (vpn_chamfer_loss.h holds the one summation order).
#include "vpn_common.h"
#include "vpn_chamfer_loss.h"

namespace {

constexpr int EV_CHUNK = 1024;       // samples of a batch the finishing workgroup stages in LDS at a time

inline size_t ev_doubles(int C) { return 3 + 2 * (size_t)C; }
inline size_t ev_counts(int C) { return 2 + (size_t)C; }

// One workgroup (256 lanes) per sample.  Which workgroup finishes the batch varies from run to run; what it computes does
// not: every sum below has one fixed order, and nothing is accumulated with a floating-point atomic.
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float* __restrict__ d1, const float* __restrict__ d2,
                                                              const float* __restrict__ emd_dist,
                                                              const int32_t* __restrict__ class_index, int B, int N, int M,
                                                              int C, float w1, float w2, float cd_scale,
                                                              double* state, float* cd_b, float* emd_b) {
    __shared__ float red[2][4];
    __shared__ double dred[4];
    __shared__ int is_last;
    __shared__ float s_cd[EV_CHUNK], s_emd[EV_CHUNK];
    __shared__ int s_cls[EV_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- this sample: cd_b as vpn_chamfer_loss gives it (x cd_scale, test.py:101), emd_b = mean_i sqrtf(dist_i)
    // (test_gcn.py:83) summed in fp64 -- lane t owns elements t, t + 256, ...; xor tree over the wave; the four waves in
    // order -- and rounded to fp32 once
    const float loss = vpn::chamfer_sample_loss_256(d1 + (size_t)b * N, d2 + (size_t)b * M, N, M, w1, w2, red);
    if (emd_dist) {
        const float* row = emd_dist + (size_t)b * N;
        double acc = 0.0;
        for (int i = tid; i < N; i += 256) acc += (double)sqrtf(row[i]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) dred[wave] = acc;
    }
    __syncthreads();
    int* ticket = reinterpret_cast<int*>(state + 2);
    if (tid == 0) {
        __hip_atomic_store(cd_b + b, loss * cd_scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (emd_dist) {
            const double s = (dred[0] + dred[1]) + (dred[2] + dred[3]);
            __hip_atomic_store(emd_b + b, (float)(s / (double)N), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // publish, then arrive (the hand-off of loss_finalize_kernel in raster.hip): release, wait for it, relaxed add
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = old == B - 1;
        if (is_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!is_last) return;

    // ---- the batch is complete: the bookkeeping of test_gcn.py:145-152 in fp64.  Lane c owns class c (c + 256, ...) and
    // walks the samples in order b = 0 .. B-1, which is the order Python's `+= x.item()` adds in; lane 255 forms the two
    // batch means and counts the samples whose class is outside [0, C).
    double* sum_cd = state + 3;
    double* sum_emd = state + 3 + C;
    long long* counts = reinterpret_cast<long long*>(state + 3 + 2 * (size_t)C);
    double tot_cd = 0.0, tot_emd = 0.0;
    long long invalid = 0;
    for (int base = 0; base < B; base += EV_CHUNK) {
        const int m = min(EV_CHUNK, B - base);
        __syncthreads();                                 // the previous chunk has been read
        for (int i = tid; i < m; i += 256) {
            s_cd[i] = __hip_atomic_load(cd_b + base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_emd[i] = emd_dist ? __hip_atomic_load(emd_b + base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
            s_cls[i] = class_index[base + i];
        }
        __syncthreads();
        for (int c = tid; c < C; c += 256) {
            double a = sum_cd[c], e = sum_emd[c];
            long long k = counts[2 + c];
            for (int i = 0; i < m; ++i) {
                if (s_cls[i] == c) { a += (double)s_cd[i]; e += (double)s_emd[i]; ++k; }
            }
            sum_cd[c] = a;
            sum_emd[c] = e;
            counts[2 + c] = k;
        }
        if (tid == 255) {
            for (int i = 0; i < m; ++i) {
                tot_cd += (double)s_cd[i];
                tot_emd += (double)s_emd[i];
                invalid += (unsigned)s_cls[i] >= (unsigned)C;
            }
        }
    }
    if (tid == 255) {
        state[0] += tot_cd / (double)B;
        state[1] += tot_emd / (double)B;
        counts[0] += 1;
        counts[1] += invalid;
    }
    if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next call / replay
}

}  // namespace

extern "C" size_t vpn_eval_state_size(int num_classes) {
    if (num_classes <= 0) return 0;
    return (ev_doubles(num_classes) + ev_counts(num_classes)) * 8;
}

extern "C" int vpn_eval_accumulate(const float* dist1, const float* dist2, const float* emd_dist,
                                   const int32_t* class_index, int B, int N, int M, int num_classes, float w1, float w2,
                                   float cd_scale, void* state, float* cd_b, float* emd_b, void* stream) {
    if (!dist1 || !dist2 || !class_index || !state || !cd_b) return VPN_E_BADARG;
    if (emd_dist && !emd_b) return VPN_E_BADARG;
    if (B <= 0 || N <= 0 || M <= 0 || num_classes <= 0) return VPN_E_BADARG;
    if (emd_dist && N != M) return VPN_E_BADARG;                 // the auction pairs equal clouds (emd_module.py:36)
    if (reinterpret_cast<uintptr_t>(state) & 7) return VPN_E_BADARG;
    VPN_LAUNCH(eval_accumulate_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, dist1, dist2, emd_dist, class_index, B, N,
               M, num_classes, w1, w2, cd_scale, static_cast<double*>(state), cd_b, emd_b);
    VPN_LAUNCH_CHECK();
    return 0;
}
