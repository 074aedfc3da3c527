// vpn_chamfer_loss.h — the per-sample Chamfer loss of chamfer_distance.py:25-28 as ONE device function, so that every
// kernel that reports it (chamfer_loss_kernel in chamfer.hip, eval_accumulate_kernel in evaluate.hip) sums in the same
// order and rounds in the same places: the same bits for the same dist1 / dist2 / w1 / w2.  Files that include this are
// built with -ffp-contract=off (build.py); the pragma below says so again for this function.
#pragma once
#include "vpn_common.h"

namespace vpn {

// sum of n floats by one workgroup of 256 lanes: float4 loads when the row is 16-byte aligned, 4 independent
// accumulators so the loads pipeline; fixed summation order (deterministic)
__device__ inline float row_sum_256(const float* __restrict__ p, int n) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) { const float4 v = p4[i]; a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w; }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += 256) a0 += p[i];
    return (a0 + a1) + (a2 + a3);
}

// loss = w1 * mean(d1[0..N)) + w2 * mean(d2[0..M)) by a workgroup of 256 lanes (four waves); red: 8 floats of LDS.
// Every lane must call it (it holds a barrier); the value is returned in thread 0 only.
__device__ inline float chamfer_sample_loss_256(const float* __restrict__ d1, const float* __restrict__ d2, int N, int M,
                                                float w1, float w2, float (*red)[4]) {
#pragma clang fp contract(off)
    float s1 = wave_sum(row_sum_256(d1, N));
    float s2 = wave_sum(row_sum_256(d2, M));
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    float loss = 0.f;
    if (threadIdx.x == 0) {
        float a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        float c = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        loss = w1 * (a / (float)N) + w2 * (c / (float)M);
    }
    return loss;
}

}  // namespace vpn
