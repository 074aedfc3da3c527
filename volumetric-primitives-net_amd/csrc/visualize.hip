// visualize.hip — the visualisation stage (gfx950): colour renders of all views of all samples in one launch.
//
// Replaces (reference file:line) the render loop of the visual dumps: modules/visualize/render.py:13-24 (one DIBRenderer
// call of batch one per view, each followed by .cpu()), driven by vp_mesh.py:14-32 (13 or 37 renders per GIF), mesh.py:7-50
// and vp_mesh.py:73-92.  DIBRenderer lives in kaolin, which is absent: pixel values are parity-unpinned; the contract is the
// camera (vpn_raster_common.h make_camera, the pixel grid of the primitive raster) and the specification in DESIGN.md 4.10,
// restated in PyTorch by tests/visualize_ref.py.
//
// Both kernels are forward only and write uint8 RGB (HWC) straight into a caller-owned frame buffer: view (s, v) goes to
//   frames + view_offset[s * V + v] + row * pitch + col * 3
// so the strip of a GIF frame is assembled by the kernel.  A view whose rectangle does not lie inside [0, frames_bytes) is
// not written at all (the offsets are device data: they are checked where they are used).
//
//   vis_primitives_kernel  exact ray / primitive entry depths in each primitive's scaled frame (the notation of
//                          oracle.raster), nearest hit wins, flat or headlight-shaded palette colours
//   vis_mesh_kernel        z-buffered triangles with perspective-correct vertex colours; faces are rejected per tile by
//                          their projected bounding box and the survivors compacted into LDS before the per-pixel loop
//
// One workgroup (256 lanes) per (sample, view, 32x32 pixel tile); a lane owns one column and four rows of the tile.
// The hit arithmetic is compiled without contraction: every operation is rounded by itself, in the order the restatement
// uses, so that the two decide "which primitive is in front" from the same numbers.
#include "vpn_raster_common.h"

namespace vpn {

constexpr int V_T = 32;                   // tile edge in pixels
constexpr int V_PPL = 4;                  // pixels per lane: rows r, r + 8, r + 16, r + 24 of one column
constexpr float V_NEAR = 1e-3f;           // oracle MESH_NEAR: nothing closer to the camera plane is drawn
constexpr float V_MIN_AREA2 = 1e-12f;     // oracle MESH_MIN_AREA2
constexpr int V_REC = 7;                  // float4 per primitive in LDS: (o~ | kind), Mr, Mu, Mf, three normal columns | palette
constexpr int V_FACE = 3;                 // float4 per staged face: (ax ay bx by), (cx cy 1/za 1/zb), (1/zc face - -)
constexpr int V_PASS = 256;               // faces tested per pass: lane = face

struct VTile {
    int sv, c0, r0, col, row0;
    float px, py[V_PPL];                  // ray slopes of the lane's pixel centres (oracle.pixel_grid)
};

__device__ inline VTile vis_tile(int H, int W, int tiles_x, int tiles) {
#pragma clang fp contract(off)
    VTile T;
    const int id = blockIdx.x;
    T.sv = id / tiles;
    const int pt = id - T.sv * tiles;
    const int ty = pt / tiles_x, tx = pt - ty * tiles_x;
    T.c0 = tx * V_T; T.r0 = ty * V_T;
    T.col = T.c0 + (threadIdx.x & 31);
    T.row0 = T.r0 + (threadIdx.x >> 5);
    const float txs = R_TAN_HALF_FOV * (float)W / (float)H;
    T.px = ((2.0f * ((float)T.col + 0.5f) / (float)W) - 1.0f) * txs;
#pragma unroll
    for (int s = 0; s < V_PPL; ++s) T.py[s] = (1.0f - (2.0f * ((float)(T.row0 + 8 * s) + 0.5f) / (float)H)) * R_TAN_HALF_FOV;
    return T;
}

// ToPILImage's quantisation after a clamp: [0,1] -> 0..255, truncated
__device__ inline unsigned char vis_q(float x) {
#pragma clang fp contract(off)
    return (unsigned char)(int)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f);
}

// destination of view sv, or nullptr when its rectangle would leave the frame buffer
__device__ inline unsigned char* vis_dest(unsigned char* frames, long long frames_bytes, long long pitch,
                                          const long long* __restrict__ view_offset, int sv, int H, int W) {
    const long long off = view_offset ? view_offset[sv] : (long long)sv * H * pitch;
    const long long last = off + (long long)(H - 1) * pitch + (long long)W * 3;
    if (off < 0 || pitch < (long long)W * 3 || last > frames_bytes) return nullptr;
    return frames + off;
}

__device__ inline void vis_store(unsigned char* dst, long long pitch, int row, int col, float r, float g, float b) {
    unsigned char* p = dst + (long long)row * pitch + (long long)col * 3;
    p[0] = vis_q(r); p[1] = vis_q(g); p[2] = vis_q(b);
}

// ---------------------------------------------------------------------------------------------------------------
// primitives
__global__ __launch_bounds__(256) void vis_primitives_kernel(const float* __restrict__ params, const int32_t* __restrict__ kinds,
                                                             const float* __restrict__ cams, const float* __restrict__ palette,
                                                             int K, int V, int H, int W, int tiles_x, int tiles, float ambient,
                                                             float bg0, float bg1, float bg2, unsigned char* frames,
                                                             long long frames_bytes, long long pitch,
                                                             const long long* __restrict__ view_offset) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float4 vis_lds[];       // K * V_REC records, then K visibility flags
    __shared__ Camera C;
    float4* rec = vis_lds;
    int* svis = reinterpret_cast<int*>(vis_lds + (size_t)K * V_REC);
    const VTile T = vis_tile(H, W, tiles_x, tiles);
    const int s = T.sv / V;
    if (threadIdx.x == 0) C = make_camera(cams + (size_t)T.sv * 3);
    __syncthreads();
    // the records of this (sample, view), once per workgroup: lane = primitive
    for (int k = threadIdx.x; k < K; k += 256) {
        const float* prm = params + ((size_t)s * K + k) * VPN_PARAM_STRIDE;
        const int kind = kinds[k] == VPN_SPHERE ? VPN_SPHERE : VPN_CUBOID;
        const Pose P = make_pose(prm[3], prm[4], prm[5], prm[6]);
        float4 full[R_REC];
        make_record_from(C, P, prm, kind, H, W, 0.0f, full);              // sigma 0: the region m2 <= 1.004, a superset of the hits
        float4* r = rec + (size_t)k * V_REC;
        r[0] = full[0]; r[1] = full[1]; r[2] = full[2]; r[3] = full[3];
        const float* pal = palette + (size_t)k * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                                     // column a of R over v_a: gradient of the scaled frame's coordinate a
            const float iv = 1.0f / prm[a];
            r[4 + a] = make_float4(P.R.m[0][a] * iv, P.R.m[1][a] * iv, P.R.m[2][a] * iv, pal[a]);
        }
        svis[k] = prim_hits_tile(kind, full + 4, T.c0, T.r0, H, W, V_T, V_T) ? 1 : 0;
    }
    __syncthreads();

    float zb[V_PPL];
    int kb[V_PPL];
#pragma unroll
    for (int i = 0; i < V_PPL; ++i) { zb[i] = 3.0e38f; kb[i] = -1; }
    for (int k = 0; k < K; ++k) {
        if (!svis[k]) continue;                                           // uniform over the workgroup
        const float4 ro = rec[k * V_REC], mr = rec[k * V_REC + 1], mu = rec[k * V_REC + 2], mf = rec[k * V_REC + 3];
        const float ex = mf.x + T.px * mr.x, ey = mf.y + T.px * mr.y, ez = mf.z + T.px * mr.z;
        const bool box = __float_as_int(ro.w) != VPN_SPHERE;
#pragma unroll
        for (int i = 0; i < V_PPL; ++i) {
            const float dx = ex + T.py[i] * mu.x, dy = ey + T.py[i] * mu.y, dz = ez + T.py[i] * mu.z;
            float z;
            bool hit;
            if (!box) {
                const float A = (dx * dx + dy * dy) + dz * dz;
                const float Bq = (ro.x * dx + ro.y * dy) + ro.z * dz;
                const float ss = -Bq / A;
                const float wx = ro.x + ss * dx, wy = ro.y + ss * dy, wz = ro.z + ss * dz;
                const float u = 1.0f - ((wx * wx + wy * wy) + wz * wz);
                hit = u > 0.0f;
                z = ss - sqrtf(fmaxf(u, 0.0f) / A);
            } else {
                const float gx = dx < 0.0f ? -1.0f : 1.0f, gy = dy < 0.0f ? -1.0f : 1.0f, gz = dz < 0.0f ? -1.0f : 1.0f;
                const float sx = fabsf(dx) < R_EPS_D ? gx * R_EPS_D : dx, sy = fabsf(dy) < R_EPS_D ? gy * R_EPS_D : dy;
                const float sz = fabsf(dz) < R_EPS_D ? gz * R_EPS_D : dz;
                const float n0 = (-gx - ro.x) / sx, n1 = (-gy - ro.y) / sy, n2 = (-gz - ro.z) / sz;
                const float f0 = (gx - ro.x) / sx, f1 = (gy - ro.y) / sy, f2 = (gz - ro.z) / sz;
                float tn = n1 > n0 ? n1 : n0;
                tn = n2 > tn ? n2 : tn;
                float tf = f1 < f0 ? f1 : f0;
                tf = f2 < tf ? f2 : tf;
                hit = tn <= tf;
                z = tn;
            }
            if (hit && z > V_NEAR && z < zb[i]) { zb[i] = z; kb[i] = k; }   // strict: equal depths stay with the lower index
        }
    }

    unsigned char* dst = vis_dest(frames, frames_bytes, pitch, view_offset, T.sv, H, W);
    if (!dst || T.col >= W) return;
#pragma unroll
    for (int i = 0; i < V_PPL; ++i) {
        const int row = T.row0 + 8 * i;
        if (row >= H) continue;
        if (kb[i] < 0) { vis_store(dst, pitch, row, T.col, bg0, bg1, bg2); continue; }
        const int k = kb[i];
        const float4 ro = rec[k * V_REC], mr = rec[k * V_REC + 1], mu = rec[k * V_REC + 2], mf = rec[k * V_REC + 3];
        const float4 c0 = rec[k * V_REC + 4], c1 = rec[k * V_REC + 5], c2 = rec[k * V_REC + 6];
        const float dx = (mf.x + T.px * mr.x) + T.py[i] * mu.x, dy = (mf.y + T.px * mr.y) + T.py[i] * mu.y;
        const float dz = (mf.z + T.px * mr.z) + T.py[i] * mu.z;
        float g0, g1, g2;                                                 // gradient of the surface function in the scaled frame
        if (__float_as_int(ro.w) == VPN_SPHERE) {
            g0 = ro.x + zb[i] * dx; g1 = ro.y + zb[i] * dy; g2 = ro.z + zb[i] * dz;
        } else {                                                          // the slab of t_near (lowest axis on ties), facing the eye
            const float gx = dx < 0.0f ? -1.0f : 1.0f, gy = dy < 0.0f ? -1.0f : 1.0f, gz = dz < 0.0f ? -1.0f : 1.0f;
            const float sx = fabsf(dx) < R_EPS_D ? gx * R_EPS_D : dx, sy = fabsf(dy) < R_EPS_D ? gy * R_EPS_D : dy;
            const float sz = fabsf(dz) < R_EPS_D ? gz * R_EPS_D : dz;
            const float n0 = (-gx - ro.x) / sx, n1 = (-gy - ro.y) / sy, n2 = (-gz - ro.z) / sz;
            int ax = n1 > n0 ? 1 : 0;
            const float tn = n1 > n0 ? n1 : n0;
            ax = n2 > tn ? 2 : ax;
            g0 = ax == 0 ? -gx : 0.0f; g1 = ax == 1 ? -gy : 0.0f; g2 = ax == 2 ? -gz : 0.0f;
        }
        const float nx = (g0 * c0.x + g1 * c1.x) + g2 * c2.x, ny = (g0 * c0.y + g1 * c1.y) + g2 * c2.y;
        const float nz = (g0 * c0.z + g1 * c1.z) + g2 * c2.z;
        const float wx = (C.fwd[0] + T.px * C.right[0]) + T.py[i] * C.up[0], wy = (C.fwd[1] + T.px * C.right[1]) + T.py[i] * C.up[1];
        const float wz = (C.fwd[2] + T.px * C.right[2]) + T.py[i] * C.up[2];
        const float nn = sqrtf((nx * nx + ny * ny) + nz * nz), wn = sqrtf((wx * wx + wy * wy) + wz * wz);
        const float cosv = -(((nx * wx + ny * wy) + nz * wz) / (nn * wn));
        const float shade = ambient + (1.0f - ambient) * fmaxf(cosv, 0.0f);
        vis_store(dst, pitch, row, T.col, c0.w * shade, c1.w * shade, c2.w * shade);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// triangle meshes

// projection of every vertex for every (sample, view): oracle.mesh_project
__global__ __launch_bounds__(256) void vis_project_kernel(const float* __restrict__ verts, const float* __restrict__ cams, int V,
                                                          int P, float4* __restrict__ proj) {
#pragma clang fp contract(off)
    __shared__ Camera C;
    const int sv = blockIdx.y, s = sv / V;
    if (threadIdx.x == 0) C = make_camera(cams + (size_t)sv * 3);
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const F3 v = ld3(verts + ((size_t)s * P + p) * 3);
    const float rx = v.x - C.eye[0], ry = v.y - C.eye[1], rz = v.z - C.eye[2];
    const float xc = (rx * C.right[0] + ry * C.right[1]) + rz * C.right[2];
    const float yc = (rx * C.up[0] + ry * C.up[1]) + rz * C.up[2];
    const float zc = (rx * C.fwd[0] + ry * C.fwd[1]) + rz * C.fwd[2];
    const float zs = zc > V_NEAR ? zc : 1.0f;
    const float den = zs * R_TAN_HALF_FOV;
    proj[(size_t)sv * P + p] = make_float4(xc / den, yc / den, zc, 0.0f);
}

__global__ __launch_bounds__(256) void vis_mesh_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                       const float* __restrict__ colors, const float* __restrict__ cams,
                                                       const float4* __restrict__ proj, int V, int P, int F, int H, int W,
                                                       int tiles_x, int tiles, float ambient, float bg0, float bg1, float bg2,
                                                       unsigned char* frames, long long frames_bytes, long long pitch,
                                                       const long long* __restrict__ view_offset) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float4 sface[V_PASS * V_FACE];
    __shared__ int wcount[4];
    __shared__ Camera C;
    const VTile T = vis_tile(H, W, tiles_x, tiles);
    const int s = T.sv / V, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) C = make_camera(cams + (size_t)T.sv * 3);
    __syncthreads();
    const float4* proj_v = proj + (size_t)T.sv * P;
    const float ar = (float)W / (float)H;
    // pixel centres and the tile's rectangle in NDC (oracle.mesh_raster: the pixel grid over tan(fov / 2))
    const float gx = T.px / R_TAN_HALF_FOV;
    float gy[V_PPL];
#pragma unroll
    for (int i = 0; i < V_PPL; ++i) gy[i] = T.py[i] / R_TAN_HALF_FOV;
    const float tx0 = ((2.0f * (float)T.c0 / (float)W) - 1.0f) * ar, tx1 = ((2.0f * (float)(T.c0 + V_T) / (float)W) - 1.0f) * ar;
    const float ty1 = 1.0f - (2.0f * (float)T.r0 / (float)H), ty0 = 1.0f - (2.0f * (float)(T.r0 + V_T) / (float)H);

    float zb[V_PPL], la[V_PPL], lb[V_PPL];      // best depth and the screen-space weights of corners a, b at the winner
    int fb[V_PPL];
#pragma unroll
    for (int i = 0; i < V_PPL; ++i) { zb[i] = 3.0e38f; fb[i] = -1; la[i] = lb[i] = 0.0f; }

    for (int f0 = 0; f0 < F; f0 += V_PASS) {
        // lane = face: gather, near test, bounding box against the tile; survivors keep their order in LDS
        const int f = f0 + (int)threadIdx.x;
        bool vis = false;
        float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A, Cc = A;
        if (f < F) {
            // vertex indices are data: clamped, so that a bad face can neither fault nor reach another sample's vertices
            const int ia = min(max(faces[f * 3], 0), P - 1), ib = min(max(faces[f * 3 + 1], 0), P - 1), ic = min(max(faces[f * 3 + 2], 0), P - 1);
            A = proj_v[ia]; B = proj_v[ib]; Cc = proj_v[ic];
            const bool ok = A.z > V_NEAR && B.z > V_NEAR && Cc.z > V_NEAR;
            const float x0 = fminf(fminf(A.x, B.x), Cc.x), x1 = fmaxf(fmaxf(A.x, B.x), Cc.x);
            const float y0 = fminf(fminf(A.y, B.y), Cc.y), y1 = fmaxf(fmaxf(A.y, B.y), Cc.y);
            vis = ok && x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
        }
        const unsigned long long m = __ballot(vis);
        if (lane == 0) wcount[wave] = __builtin_popcountll(m);
        __syncthreads();
        int base = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) base += w < wave ? wcount[w] : 0;
        const int n = (wcount[0] + wcount[1]) + (wcount[2] + wcount[3]);
        if (vis) {
            const int slot = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            sface[slot * V_FACE] = make_float4(A.x, A.y, B.x, B.y);
            sface[slot * V_FACE + 1] = make_float4(Cc.x, Cc.y, 1.0f / A.z, 1.0f / B.z);
            sface[slot * V_FACE + 2] = make_float4(1.0f / Cc.z, __int_as_float(f), 0.0f, 0.0f);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 q0 = sface[j * V_FACE], q1 = sface[j * V_FACE + 1], q2 = sface[j * V_FACE + 2];
            const float ax = q0.x, ay = q0.y, bx = q0.z, by = q0.w, cx = q1.x, cy = q1.y;
#pragma unroll
            for (int i = 0; i < V_PPL; ++i) {
                const float e0 = (bx - ax) * (gy[i] - ay) - (by - ay) * (gx - ax);
                const float e1 = (cx - bx) * (gy[i] - by) - (cy - by) * (gx - bx);
                const float e2 = (ax - cx) * (gy[i] - cy) - (ay - cy) * (gx - cx);
                const float area2 = (e0 + e1) + e2;
                const bool inside = ((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f)) && fabsf(area2) > V_MIN_AREA2;
                // corner a is opposite edge (b, c), b opposite (c, a), c opposite (a, b); 1/z is linear in screen space
                const float wa = e1 / area2, wb = e2 / area2, wc = e0 / area2;
                const float iz = (wa * q1.z + wb * q1.w) + wc * q2.x;
                const float z = 1.0f / iz;
                if (inside && z < zb[i]) { zb[i] = z; fb[i] = __float_as_int(q2.y); la[i] = wa; lb[i] = wb; }
            }
        }
        __syncthreads();                                                  // the next pass overwrites sface and wcount
    }

    unsigned char* dst = vis_dest(frames, frames_bytes, pitch, view_offset, T.sv, H, W);
    if (!dst || T.col >= W) return;
    const float* vb = verts + (size_t)s * P * 3;
    const float* cb = colors + (size_t)s * P * 3;
#pragma unroll
    for (int i = 0; i < V_PPL; ++i) {
        const int row = T.row0 + 8 * i;
        if (row >= H) continue;
        if (fb[i] < 0) { vis_store(dst, pitch, row, T.col, bg0, bg1, bg2); continue; }
        const int f = fb[i];
        const int ia = min(max(faces[f * 3], 0), P - 1), ib = min(max(faces[f * 3 + 1], 0), P - 1), ic = min(max(faces[f * 3 + 2], 0), P - 1);
        const float wa = la[i], wb = lb[i], wc = (1.0f - wa) - wb;
        const float za = proj_v[ia].z, zb_ = proj_v[ib].z, zc = proj_v[ic].z;
        const float ua = wa / za * zb[i], ub = wb / zb_ * zb[i], uc = wc / zc * zb[i];          // c / z linear, times z
        const F3 ca = ld3(cb + ia * 3), cbv = ld3(cb + ib * 3), cc = ld3(cb + ic * 3);
        float shade = 1.0f;
        if (ambient != 1.0f) {                                            // headlight on the unit face normal, two-sided
            const F3 pa = ld3(vb + ia * 3), pb = ld3(vb + ib * 3), pc = ld3(vb + ic * 3);
            const float ux = pb.x - pa.x, uy = pb.y - pa.y, uz = pb.z - pa.z, vx = pc.x - pa.x, vy = pc.y - pa.y, vz = pc.z - pa.z;
            const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const float wx = (C.fwd[0] + T.px * C.right[0]) + T.py[i] * C.up[0], wy = (C.fwd[1] + T.px * C.right[1]) + T.py[i] * C.up[1];
            const float wz = (C.fwd[2] + T.px * C.right[2]) + T.py[i] * C.up[2];
            const float nn = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-20f), wn = sqrtf((wx * wx + wy * wy) + wz * wz);
            shade = ambient + (1.0f - ambient) * fabsf(((nx * wx + ny * wy) + nz * wz) / (nn * wn));
        }
        vis_store(dst, pitch, row, T.col, ((ua * ca.x + ub * cbv.x) + uc * cc.x) * shade, ((ua * ca.y + ub * cbv.y) + uc * cc.y) * shade,
                  ((ua * ca.z + ub * cbv.z) + uc * cc.z) * shade);
    }
}

}  // namespace vpn

using namespace vpn;

static int vis_args(const void* a, const void* b, const void* cams, const void* frames, int S, int V, int H, int W, long long pitch,
                    size_t frames_bytes, const void* view_offset, long long* tiles_out) {
    if (!a || !b || !cams || !frames) return VPN_E_BADARG;
    if (S <= 0 || V <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    if (pitch < (long long)W * 3) return VPN_E_BADARG;
    if (H > 16384 || W > 16384) return VPN_E_TOOBIG;
    const long long tiles = (long long)((W + V_T - 1) / V_T) * ((H + V_T - 1) / V_T);
    if ((long long)S * V > 65535 || (long long)S * V * tiles > 0x7fffffffLL) return VPN_E_TOOBIG;
    // dense layout (no offsets): every view must fit; with offsets the kernel checks each view where it writes
    if (!view_offset && (unsigned long long)S * V * H * (unsigned long long)pitch > (unsigned long long)frames_bytes) return VPN_E_BADARG;
    *tiles_out = tiles;
    return 0;
}

extern "C" int vpn_vis_primitives(const float* params, const int32_t* kinds, const float* cams, const float* palette, int S, int K,
                                  int V, int H, int W, float ambient, float bg_r, float bg_g, float bg_b, uint8_t* frames,
                                  size_t frames_bytes, long long pitch, const long long* view_offset, void* stream) {
    long long tiles = 0;
    if (!palette || K <= 0) return VPN_E_BADARG;
    int rc = vis_args(params, kinds, cams, frames, S, V, H, W, pitch, frames_bytes, view_offset, &tiles);
    if (rc) return rc;
    if (!(ambient >= 0.0f && ambient <= 1.0f)) return VPN_E_BADARG;
    if (K > VPN_VIS_MAX_PRIMS) return VPN_E_TOOBIG;
    const size_t lds = (size_t)K * V_REC * sizeof(float4) + (size_t)K * sizeof(int);
    const int tiles_x = (W + V_T - 1) / V_T;
    VPN_LAUNCH(vis_primitives_kernel, dim3((unsigned)((long long)S * V * tiles)), dim3(256), lds, (hipStream_t)stream, params, kinds,
               cams, palette, K, V, H, W, tiles_x, (int)tiles, ambient, bg_r, bg_g, bg_b, frames, (long long)frames_bytes, pitch,
               view_offset);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vpn_vis_mesh_workspace(int S, int V, int P) {
    if (S <= 0 || V <= 0 || P <= 0) return 0;
    return (size_t)S * V * P * sizeof(float4);                            // the projected vertices of every (sample, view)
}

extern "C" int vpn_vis_mesh(const float* verts, const int32_t* faces, const float* colors, const float* cams, int S, int P, int F,
                            int V, int H, int W, float ambient, float bg_r, float bg_g, float bg_b, void* workspace, uint8_t* frames,
                            size_t frames_bytes, long long pitch, const long long* view_offset, void* stream) {
    long long tiles = 0;
    if (!colors || !workspace || P <= 0 || F <= 0 || ((uintptr_t)workspace & 15) != 0) return VPN_E_BADARG;
    int rc = vis_args(verts, faces, cams, frames, S, V, H, W, pitch, frames_bytes, view_offset, &tiles);
    if (rc) return rc;
    if (!(ambient >= 0.0f && ambient <= 1.0f)) return VPN_E_BADARG;
    if ((long long)S * V * P > 0x7fffffffLL / 4 || (long long)F > 0x7fffffffLL / 3) return VPN_E_TOOBIG;
    hipStream_t st = (hipStream_t)stream;
    float4* proj = (float4*)workspace;
    VPN_LAUNCH(vis_project_kernel, dim3((P + 255) / 256, S * V), dim3(256), 0, st, verts, cams, V, P, proj);
    VPN_LAUNCH_CHECK();
    const int tiles_x = (W + V_T - 1) / V_T;
    VPN_LAUNCH(vis_mesh_kernel, dim3((unsigned)((long long)S * V * tiles)), dim3(256), 0, st, verts, faces, colors, cams,
               (const float4*)proj, V, P, F, H, W, tiles_x, (int)tiles, ambient, bg_r, bg_g, bg_b, frames, (long long)frames_bytes,
               pitch, view_offset);
    VPN_LAUNCH_CHECK();
    return 0;
}
