// occupancy_prim.h — the pose record of a primitive and the local coordinates of a point in it, shared by occupancy.hip
// (inside / outside) and isosurface.hip (the implicit field).  Both files are built with
// -ffp-contract=off and every operation below is rounded by itself, so the two kernels form the same x~ bit for bit and
// (field <= 0) is the occupancy.
#pragma once
#include "vpn_common.h"

namespace vpn {

constexpr int OC_STAGE = 256;                        // primitives staged in LDS at a time: one per lane

struct OcPrim { float r[9]; float tx, ty, tz, vx, vy, vz; int sphere; };

// the record of primitive k of sample b: make_pose, the sampler's and the raster's own function
__device__ inline void oc_stage_prim(OcPrim& p, const float* __restrict__ params, const int32_t* __restrict__ kinds, int b, int K,
                                     int k) {
    const float* prm = params + ((size_t)b * K + k) * VPN_PARAM_STRIDE;
    const Pose pose = make_pose(prm[3], prm[4], prm[5], prm[6]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.r[r * 3 + c] = pose.R.m[r][c];
    }
    p.vx = prm[0]; p.vy = prm[1]; p.vz = prm[2];
    p.tx = prm[7]; p.ty = prm[8]; p.tz = prm[9];
    p.sphere = kinds[k] == VPN_SPHERE;
}

// x~ = R^T (x - t) / v
__device__ inline F3 oc_local(const OcPrim& p, F3 x) {
    const float dx = x.x - p.tx, dy = x.y - p.ty, dz = x.z - p.tz;
    return F3{(p.r[0] * dx + p.r[3] * dy + p.r[6] * dz) / p.vx,       // R^T d: column i of R
              (p.r[1] * dx + p.r[4] * dy + p.r[7] * dz) / p.vy,
              (p.r[2] * dx + p.r[5] * dy + p.r[8] * dz) / p.vz};
}

}  // namespace vpn
