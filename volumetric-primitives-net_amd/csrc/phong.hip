// phong.hip — textured, lit renders of all views of all scenes of a triangle mesh in one launch (gfx950).
//
// Replaces (reference file:line) modules/render/phong_renderer.py:12-38: one freshly constructed DIBRenderer(mode='Phong')
// call per view, each followed by .cpu() (generate.py:150-161, point_mixup.py:58-70).  DIBRenderer is kaolin's, which is
// absent: pixel values are parity-unpinned; the contract is the camera (vpn_raster_common.h make_camera), the mesh rule of
// DESIGN.md 4.10 for "which face is seen" and the shading specification of DESIGN.md 4.11, restated in PyTorch by
// tests/phong_ref.py.
//
//   phong_project_kernel  oracle.mesh_project of every vertex for every (scene, view), as vis_project_kernel
//   phong_mesh_kernel     the tile walk of vis_mesh_kernel (visualize.hip): faces rejected per tile by their projected
//                         bounding box, the survivors compacted in order into LDS 256 per pass, nearest face wins and equal
//                         depths stay with the lowest face; then, once per pixel and for the winner only, the texture
//                         coordinate (perspective-correct), a nearest-texel lookup and Phong lighting on the unit face
//                         normal, written as float RGB
//
// One workgroup (256 lanes) per (scene, view, 32x32 pixel tile); a lane owns one column and four rows of the tile.  The walk
// is a copy, not a shared header: vis_mesh_kernel's code and resource figures stay what they are.  Compiled without
// contraction, so that depth decisions round like the restatement.
#include "vpn_raster_common.h"

namespace vpn {

constexpr int P_T = 32;                   // tile edge in pixels
constexpr int P_PPL = 4;                  // pixels per lane: rows r, r + 8, r + 16, r + 24 of one column
constexpr float P_NEAR = 1e-3f;           // oracle MESH_NEAR
constexpr float P_MIN_AREA2 = 1e-12f;     // oracle MESH_MIN_AREA2
constexpr int P_FACE = 3;                 // float4 per staged face: (ax ay bx by), (cx cy 1/za 1/zb), (1/zc face - -)
constexpr int P_PASS = 256;               // faces tested per pass: lane = face

__global__ __launch_bounds__(256) void phong_project_kernel(const float* __restrict__ verts, const float* __restrict__ cams, int V,
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
    const float zs = zc > P_NEAR ? zc : 1.0f;
    const float den = zs * R_TAN_HALF_FOV;
    proj[(size_t)sv * P + p] = make_float4(xc / den, yc / den, zc, 0.0f);
}

__global__ __launch_bounds__(256) void phong_mesh_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                         const float* __restrict__ uv, const float* __restrict__ texture,
                                                         const float* __restrict__ cams, const float* __restrict__ light,
                                                         const float* __restrict__ material, float shininess,
                                                         const float4* __restrict__ proj, int V, int P, int F, int TH, int TW, int H,
                                                         int W, int tiles_x, int tiles, float* __restrict__ rgb) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float4 sface[P_PASS * P_FACE];
    __shared__ int wcount[4];
    __shared__ Camera C;
    const int id = blockIdx.x;
    const int sv = id / tiles;
    const int pt = id - sv * tiles;
    const int tyi = pt / tiles_x, txi = pt - tyi * tiles_x;
    const int c0 = txi * P_T, r0 = tyi * P_T;
    const int col = c0 + (threadIdx.x & 31), row0 = r0 + (threadIdx.x >> 5);
    const int s = sv / V, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) C = make_camera(cams + (size_t)sv * 3);
    __syncthreads();
    const float4* proj_v = proj + (size_t)sv * P;
    const float ar = (float)W / (float)H;
    // ray slopes of the lane's pixel centres (oracle.pixel_grid) and the same in NDC (oracle.mesh_raster)
    const float px = ((2.0f * ((float)col + 0.5f) / (float)W) - 1.0f) * (R_TAN_HALF_FOV * (float)W / (float)H);
    const float gx = px / R_TAN_HALF_FOV;
    float py[P_PPL], gy[P_PPL];
#pragma unroll
    for (int i = 0; i < P_PPL; ++i) {
        py[i] = (1.0f - (2.0f * ((float)(row0 + 8 * i) + 0.5f) / (float)H)) * R_TAN_HALF_FOV;
        gy[i] = py[i] / R_TAN_HALF_FOV;
    }
    const float tx0 = ((2.0f * (float)c0 / (float)W) - 1.0f) * ar, tx1 = ((2.0f * (float)(c0 + P_T) / (float)W) - 1.0f) * ar;
    const float ty1 = 1.0f - (2.0f * (float)r0 / (float)H), ty0 = 1.0f - (2.0f * (float)(r0 + P_T) / (float)H);

    float zb[P_PPL], la[P_PPL], lb[P_PPL];      // best depth and the screen-space weights of corners a, b at the winner
    int fb[P_PPL];
#pragma unroll
    for (int i = 0; i < P_PPL; ++i) { zb[i] = 3.0e38f; fb[i] = -1; la[i] = lb[i] = 0.0f; }

    for (int f0 = 0; f0 < F; f0 += P_PASS) {
        // lane = face: gather, near test, bounding box against the tile; survivors keep their order in LDS
        const int f = f0 + (int)threadIdx.x;
        bool vis = false;
        float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A, Cc = A;
        if (f < F) {
            // vertex indices are data: clamped, so that a bad face can neither fault nor reach another scene's vertices
            const int ia = min(max(faces[f * 3], 0), P - 1), ib = min(max(faces[f * 3 + 1], 0), P - 1), ic = min(max(faces[f * 3 + 2], 0), P - 1);
            A = proj_v[ia]; B = proj_v[ib]; Cc = proj_v[ic];
            const bool ok = A.z > P_NEAR && B.z > P_NEAR && Cc.z > P_NEAR;
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
            sface[slot * P_FACE] = make_float4(A.x, A.y, B.x, B.y);
            sface[slot * P_FACE + 1] = make_float4(Cc.x, Cc.y, 1.0f / A.z, 1.0f / B.z);
            sface[slot * P_FACE + 2] = make_float4(1.0f / Cc.z, __int_as_float(f), 0.0f, 0.0f);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 q0 = sface[j * P_FACE], q1 = sface[j * P_FACE + 1], q2 = sface[j * P_FACE + 2];
            const float ax = q0.x, ay = q0.y, bx = q0.z, by = q0.w, cx = q1.x, cy = q1.y;
#pragma unroll
            for (int i = 0; i < P_PPL; ++i) {
                const float e0 = (bx - ax) * (gy[i] - ay) - (by - ay) * (gx - ax);
                const float e1 = (cx - bx) * (gy[i] - by) - (cy - by) * (gx - bx);
                const float e2 = (ax - cx) * (gy[i] - cy) - (ay - cy) * (gx - cx);
                const float area2 = (e0 + e1) + e2;
                const bool inside = ((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f)) && fabsf(area2) > P_MIN_AREA2;
                // corner a is opposite edge (b, c), b opposite (c, a), c opposite (a, b); 1/z is linear in screen space
                const float wa = e1 / area2, wb = e2 / area2, wc = e0 / area2;
                const float iz = (wa * q1.z + wb * q1.w) + wc * q2.x;
                const float z = 1.0f / iz;
                if (inside && z < zb[i]) { zb[i] = z; fb[i] = __float_as_int(q2.y); la[i] = wa; lb[i] = wb; }
            }
        }
        __syncthreads();                                                  // the next pass overwrites sface and wcount
    }

    if (col >= W) return;
    // the light in world space: given in the camera basis (right, up, fwd)
    const float l0 = light[0], l1 = light[1], l2 = light[2];
    float lx = (l0 * C.right[0] + l1 * C.up[0]) + l2 * C.fwd[0], ly = (l0 * C.right[1] + l1 * C.up[1]) + l2 * C.fwd[1];
    float lz = (l0 * C.right[2] + l1 * C.up[2]) + l2 * C.fwd[2];
    const float ln = fmaxf(sqrtf((lx * lx + ly * ly) + lz * lz), 1e-20f);
    lx = lx / ln; ly = ly / ln; lz = lz / ln;
    const float* vb = verts + (size_t)s * P * 3;
    const float* ub = uv + (size_t)s * P * 2;
    const float* tb = texture + (size_t)s * 3 * TH * TW;
    float* dst = rgb + (size_t)sv * H * W * 3;
#pragma unroll
    for (int i = 0; i < P_PPL; ++i) {
        const int row = row0 + 8 * i;
        if (row >= H) continue;
        float* o = dst + ((size_t)row * W + col) * 3;
        if (fb[i] < 0) { o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; continue; }
        const int f = fb[i];
        const int ia = min(max(faces[f * 3], 0), P - 1), ib = min(max(faces[f * 3 + 1], 0), P - 1), ic = min(max(faces[f * 3 + 2], 0), P - 1);
        const float wa = la[i], wb = lb[i], wc = (1.0f - wa) - wb;
        const float za = proj_v[ia].z, zb_ = proj_v[ib].z, zc = proj_v[ic].z;
        const float ka = wa / za * zb[i], kb = wb / zb_ * zb[i], kc = wc / zc * zb[i];          // uv / z linear, times z
        const float tu = (ka * ub[ia * 2] + kb * ub[ib * 2]) + kc * ub[ic * 2];
        const float tv = (ka * ub[ia * 2 + 1] + kb * ub[ib * 2 + 1]) + kc * ub[ic * 2 + 1];
        // nearest texel; the clamp is done on the float, so that no value (a NaN included) leaves the texture
        const int txl = (int)fminf(fmaxf(floorf(tu * (float)TW), 0.0f), (float)(TW - 1));
        const int tyl = (int)fminf(fmaxf(floorf(tv * (float)TH), 0.0f), (float)(TH - 1));
        const size_t tix = (size_t)tyl * TW + txl, tpl = (size_t)TH * TW;
        // unit pixel ray and unit face normal, turned towards the eye
        const float wx = (C.fwd[0] + px * C.right[0]) + py[i] * C.up[0], wy = (C.fwd[1] + px * C.right[1]) + py[i] * C.up[1];
        const float wz = (C.fwd[2] + px * C.right[2]) + py[i] * C.up[2];
        const float wn = sqrtf((wx * wx + wy * wy) + wz * wz);
        const float dx = wx / wn, dy = wy / wn, dz = wz / wn;
        const F3 pa = ld3(vb + ia * 3), pb = ld3(vb + ib * 3), pc = ld3(vb + ic * 3);
        const float ux = pb.x - pa.x, uy = pb.y - pa.y, uz = pb.z - pa.z, vx = pc.x - pa.x, vy = pc.y - pa.y, vz = pc.z - pa.z;
        float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const float nn = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-20f);
        nx = nx / nn; ny = ny / nn; nz = nz / nn;
        if ((nx * dx + ny * dy) + nz * dz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        const float cosT = fminf(fmaxf((nx * lx + ny * ly) + nz * lz, 0.0f), 1.0f);
        const float k2 = 2.0f * cosT;
        const float rx = k2 * nx - lx, ry = k2 * ny - ly, rz = k2 * nz - lz;
        const float cosA = fminf(fmaxf(-((rx * dx + ry * dy) + rz * dz), 0.0f), 1.0f);
        const float spec = powf(cosA, shininess);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float tex = tb[c * tpl + tix];
            const float val = tex * (material[c] + material[3 + c] * cosT) + material[6 + c] * spec;
            o[c] = fminf(fmaxf(val, 0.0f), 1.0f);
        }
    }
}

}  // namespace vpn

using namespace vpn;

extern "C" size_t vpn_phong_mesh_workspace(int S, int V, int P) {
    if (S <= 0 || V <= 0 || P <= 0) return 0;
    return (size_t)S * V * P * sizeof(float4);                            // the projected vertices of every (scene, view)
}

extern "C" int vpn_phong_mesh(const float* verts, const int32_t* faces, const float* uv, const float* texture, const float* cams,
                              const float* light, const float* material, float shininess, int S, int P, int F, int V, int TH, int TW,
                              int H, int W, void* workspace, float* rgb, void* stream) {
    if (!verts || !faces || !uv || !texture || !cams || !light || !material || !workspace || !rgb) return VPN_E_BADARG;
    if (((uintptr_t)workspace & 15) != 0) return VPN_E_BADARG;
    if (S <= 0 || V <= 0 || P <= 0 || F <= 0 || TH <= 0 || TW <= 0 || H <= 0 || W <= 0) return VPN_E_BADARG;
    if (!(shininess >= 0.0f)) return VPN_E_BADARG;
    if (H > 16384 || W > 16384 || TH > 16384 || TW > 16384) return VPN_E_TOOBIG;
    const long long tiles = (long long)((W + P_T - 1) / P_T) * ((H + P_T - 1) / P_T);
    if ((long long)S * V > 65535 || (long long)S * V * tiles > 0x7fffffffLL) return VPN_E_TOOBIG;
    if ((long long)S * V * P > 0x7fffffffLL / 4 || (long long)F > 0x7fffffffLL / 3) return VPN_E_TOOBIG;
    hipStream_t st = (hipStream_t)stream;
    float4* proj = (float4*)workspace;
    VPN_LAUNCH(phong_project_kernel, dim3((P + 255) / 256, S * V), dim3(256), 0, st, verts, cams, V, P, proj);
    VPN_LAUNCH_CHECK();
    const int tiles_x = (W + P_T - 1) / P_T;
    VPN_LAUNCH(phong_mesh_kernel, dim3((unsigned)((long long)S * V * tiles)), dim3(256), 0, st, verts, faces, uv, texture, cams, light,
               material, shininess, (const float4*)proj, V, P, F, TH, TW, H, W, tiles_x, (int)tiles, rgb);
    VPN_LAUNCH_CHECK();
    return 0;
}
