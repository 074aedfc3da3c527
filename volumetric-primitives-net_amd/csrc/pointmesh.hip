// pointmesh.hip — the squared distance between a point cloud and the triangles of a mesh, both ways: for
// every point the nearest face, for every face the nearest point, and the two means.  points [B,P,3], verts [B,V,3] fp32,
// ONE face list [F,3] int32 for the batch.  A brute-force pair scan: every (point, face) pair of a sample is evaluated once
// and serves both directions.
//
//   pointmesh_prep_kernel   one work-item per (face, sample): the record of the face (PmFace, 16 floats: v0, the two edges from
//                           v0, their dot products, the reciprocals of the determinant and of the three squared edge lengths;
//                           a reciprocal of something that is not > 0 is 0 and switches its candidate off).
//   pointmesh_pair_kernel   one workgroup per (tile of 256 points, slice of the faces, sample).  A work-item keeps its point in
//                           registers and walks the records of the slice; the record index is uniform, so the records come
//                           through scalar loads and cost no LDS.  Per pair pm_closest: the plane candidate (when the foot of the
//                           perpendicular lies in the triangle) and the three segment candidates, the distance of each formed
//                           from p - c, the least taken with strict < in that order.  The work-item keeps the least over the
//                           slice (strict <, ascending faces); per face the least over the wave is a butterfly of fminf and a
//                           ballot (the lowest lane that holds it), lane j keeping face j of a 64-face pass; the four waves
//                           then meet in LDS in order.  Out: partial minima [B,slices,P] and [B,tiles,F], (distance, index).
//   pointmesh_merge_kernel  one work-item per point and per face of a 256-item chunk: the partials in ascending order, strict <
//                           from (inf, 0), so ties go to the lowest index and every index is in range whatever the data hold;
//                           the chunk's two sums as in meshreg_fwd_kernel.
//   pointmesh_final_kernel  one wave: the chunk sums in a fixed order, times 1 / count.
//   pointmesh_bwd_face_kernel   one work-item per (face, sample): the gradient of the face's own dist_f record, then of every
//                           point that chose the face, found by walking face_of_point in ascending order (the address is
//                           uniform: scalar loads, sixteen in flight): [B,F,3,3].
//   pointmesh_bwd_point_kernel  one work-item per (point, sample): its own dist_p record, then every face that chose the point,
//                           by walking point_of_face.
//   pointmesh_bwd_gather_kernel one work-item per (vertex, sample): the corner gradients of its incident (face, corner) list in
//                           ascending order.
//
// The backward recomputes the closest point from the saved indices with pm_face / pm_closest, the forward's own functions.
// No atomics, no host synchronisation, nothing allocated: every minimum and sum has a fixed order, the results are bit-equal
// from run to run.  Face indices are not checked here (ops checks them on the host).
#include "vpn_common.h"

namespace vpn {

constexpr int PM_TILE = VPN_POINTMESH_TILE;        // points per workgroup of the pair scan; items per chunk of the merge
constexpr int PM_PASS = 64;                        // faces per cross-wave pass: lane j of a wave keeps face j
constexpr int PM_SCAN = 64;                        // faces (points) per workgroup of the backward's two scans: one wave
constexpr int PM_BATCH = 16;                       // entries of an index list a scan fetches at once
constexpr int PM_GATHER_BLOCK = 64;

struct PmVec { float x, y, z; };
__device__ inline PmVec pm_ld(const float* p, long long i) { const F3 f = ld3(p + 3 * i); return PmVec{f.x, f.y, f.z}; }
__device__ inline PmVec pm_sub(PmVec a, PmVec b) { return PmVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline float pm_dot(PmVec a, PmVec b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ inline float pm_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }        // NaN -> 0
__device__ inline float pm_recip(float x) { return x > 0.0f ? 1.0f / x : 0.0f; }           // 0, negative, NaN -> 0

struct __attribute__((aligned(16))) PmFace {
    float v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z;     // v0, e1 = v1 - v0, e2 = v2 - v0
    float a, b, c;                                          // e1.e1, e1.e2, e2.e2
    float inv_det, inv_a, inv_c, inv_e;                     // 1 / (a c - b^2), 1 / a, 1 / c, 1 / |v2 - v1|^2; 0 when not > 0
};
static_assert(sizeof(PmFace) == 64, "a face record is 16 floats");

struct PmHit { float d, w1, w2, rx, ry, rz; };              // squared distance, weights of v1 and v2 (w0 = 1 - w1 - w2), p - c

__device__ inline PmFace pm_face(PmVec v0, PmVec v1, PmVec v2) {
    const PmVec e1 = pm_sub(v1, v0), e2 = pm_sub(v2, v0), e3 = pm_sub(v2, v1);
    PmFace T;
    T.v0x = v0.x; T.v0y = v0.y; T.v0z = v0.z;
    T.e1x = e1.x; T.e1y = e1.y; T.e1z = e1.z;
    T.e2x = e2.x; T.e2y = e2.y; T.e2z = e2.z;
    T.a = pm_dot(e1, e1); T.b = pm_dot(e1, e2); T.c = pm_dot(e2, e2);
    T.inv_det = pm_recip(T.a * T.c - T.b * T.b);
    T.inv_a = pm_recip(T.a); T.inv_c = pm_recip(T.c); T.inv_e = pm_recip(pm_dot(e3, e3));
    return T;
}

// the face record of face f of the sample whose vertices start at v
__device__ inline PmFace pm_face_of(const float* v, const int* __restrict__ faces, int f) {
    return pm_face(pm_ld(v, faces[3 * f]), pm_ld(v, faces[3 * f + 1]), pm_ld(v, faces[3 * f + 2]));
}

// one candidate c = v0 + w1 e1 + w2 e2: kept when strictly nearer than what h holds
__device__ inline void pm_try(PmHit& h, const PmFace& T, PmVec d, float w1, float w2, bool live) {
    const float rx = fmaf(-w2, T.e2x, fmaf(-w1, T.e1x, d.x)), ry = fmaf(-w2, T.e2y, fmaf(-w1, T.e1y, d.y)),
                rz = fmaf(-w2, T.e2z, fmaf(-w1, T.e1z, d.z));
    const float q = fmaf(rz, rz, fmaf(ry, ry, rx * rx));
    if (live && q < h.d) { h.d = q; h.w1 = w1; h.w2 = w2; h.rx = rx; h.ry = ry; h.rz = rz; }
}

// the closest point of the closed triangle T to p.  Every candidate is a point of the triangle, so the result never lies
// below the true minimum; a triangle without area has no plane candidate and is the segment or point it degenerates to.
// With nothing comparable (NaN) the result is d = inf at v0.
__device__ inline PmHit pm_closest(const PmFace& T, PmVec p) {
    const PmVec d = PmVec{p.x - T.v0x, p.y - T.v0y, p.z - T.v0z};
    const float d1 = fmaf(T.e1z, d.z, fmaf(T.e1y, d.y, T.e1x * d.x)), d2 = fmaf(T.e2z, d.z, fmaf(T.e2y, d.y, T.e2x * d.x));
    PmHit h = PmHit{INFINITY, 0.0f, 0.0f, d.x, d.y, d.z};
    const float s = (T.c * d1 - T.b * d2) * T.inv_det, t = (T.a * d2 - T.b * d1) * T.inv_det;
    pm_try(h, T, d, s, t, T.inv_det > 0.0f && s >= 0.0f && t >= 0.0f && s + t <= 1.0f);
    pm_try(h, T, d, pm_clamp01(d1 * T.inv_a), 0.0f, true);                                  // v0 .. v1
    const float u = pm_clamp01((d2 - d1 - T.b + T.a) * T.inv_e);                             // v1 .. v2: (p - v1).(v2 - v1)
    pm_try(h, T, d, 1.0f - u, u, true);
    pm_try(h, T, d, 0.0f, pm_clamp01(d2 * T.inv_c), true);                                  // v0 .. v2
    return h;
}

__device__ inline float pm_wave_min(float v) {               // fminf drops a NaN when the other side is a number
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void pointmesh_prep_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             int V, int F, PmFace* __restrict__ rec) {
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= F) return;
    rec[(long long)b * F + f] = pm_face_of(verts + (long long)b * V * 3, faces, f);
}

__global__ __launch_bounds__(256) void pointmesh_pair_kernel(const float* __restrict__ points, const PmFace* __restrict__ rec,
                                                             int P, int F, int tiles, int slices, int slice_faces,
                                                             float* __restrict__ pp_d, int* __restrict__ pp_i,
                                                             float* __restrict__ pf_d, int* __restrict__ pf_i) {
    __shared__ float s_d[4][PM_PASS];
    __shared__ int s_i[4][PM_PASS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = blockIdx.x, sl = blockIdx.y, b = blockIdx.z;
    const int i = tile * PM_TILE + t;
    const bool valid = i < P;
    const PmVec p = valid ? pm_ld(points, (long long)b * P + i) : PmVec{0.0f, 0.0f, 0.0f};
    const PmFace* r = rec + (long long)b * F;
    const int f0 = sl * slice_faces, f1 = min(F, f0 + slice_faces);
    float best = INFINITY;
    int best_f = 0;
    for (int c0 = f0; c0 < f1; c0 += PM_PASS) {
        const int n = min(PM_PASS, f1 - c0);
        float keep_d = INFINITY;
        int keep_i = 0;
        for (int j = 0; j < n; ++j) {
            const PmFace T = r[c0 + j];                                        // uniform index: scalar loads
            const float q = pm_closest(T, p).d;
            const float d = valid ? q : INFINITY;
            if (d < best) { best = d; best_f = c0 + j; }
            const float m = pm_wave_min(d);
            const unsigned long long mask = __ballot(d == m);                  // empty when every lane holds a NaN
            const int src = mask ? __ffsll(mask) - 1 : 0;
            if (lane == j) { keep_d = m; keep_i = tile * PM_TILE + w * 64 + src; }
        }
        s_d[w][lane] = keep_d; s_i[w][lane] = keep_i;
        __syncthreads();
        if (t < n) {
            float bd = INFINITY;
            int bi = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (s_d[k][t] < bd) { bd = s_d[k][t]; bi = s_i[k][t]; }
            const long long o = ((long long)b * tiles + tile) * F + c0 + t;
            pf_d[o] = bd; pf_i[o] = bi;
        }
        __syncthreads();
    }
    if (valid) {
        const long long o = ((long long)b * slices + sl) * P + i;
        pp_d[o] = best; pp_i[o] = best_f;
    }
}

__global__ __launch_bounds__(256) void pointmesh_merge_kernel(const float* __restrict__ pp_d, const int* __restrict__ pp_i,
                                                              const float* __restrict__ pf_d, const int* __restrict__ pf_i,
                                                              int P, int F, int tiles, int slices, int chunks,
                                                              float* __restrict__ dist_p, int* __restrict__ face_of_point,
                                                              float* __restrict__ dist_f, int* __restrict__ point_of_face,
                                                              float* __restrict__ sums) {
    __shared__ float s_part[2][4];
    const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y, i = c * PM_TILE + t;
    float sp = 0.0f, sf = 0.0f;
    if (i < P) {
        float bd = INFINITY;
        int bi = 0;
        for (int s = 0; s < slices; ++s) {
            const long long o = ((long long)b * slices + s) * P + i;
            const float d = pp_d[o];
            if (d < bd) { bd = d; bi = pp_i[o]; }
        }
        if (dist_p) dist_p[(long long)b * P + i] = bd;
        if (face_of_point) face_of_point[(long long)b * P + i] = bi;
        sp = bd;
    }
    if (i < F) {
        float bd = INFINITY;
        int bi = 0;
        for (int s = 0; s < tiles; ++s) {
            const long long o = ((long long)b * tiles + s) * F + i;
            const float d = pf_d[o];
            if (d < bd) { bd = d; bi = pf_i[o]; }
        }
        if (dist_f) dist_f[(long long)b * F + i] = bd;
        if (point_of_face) point_of_face[(long long)b * F + i] = bi;
        sf = bd;
    }
    sp = wave_sum(sp); sf = wave_sum(sf);
    if ((t & 63) == 0) { s_part[0][t >> 6] = sp; s_part[1][t >> 6] = sf; }
    __syncthreads();
    if (t < 2) sums[((long long)b * chunks + c) * 2 + t] = ((s_part[t][0] + s_part[t][1]) + s_part[t][2]) + s_part[t][3];
}

// out [2] = the chunk sums added in a fixed order, over the number of (sample, point) and of (sample, face)
__global__ __launch_bounds__(64) void pointmesh_final_kernel(const float* __restrict__ sums, int n, float inv_p, float inv_f,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x;
    float s0 = 0.0f, s1 = 0.0f;
    for (int k = lane; k < n; k += 64) { s0 += sums[2 * (long long)k]; s1 += sums[2 * (long long)k + 1]; }
    s0 = wave_sum(s0); s1 = wave_sum(s1);
    if (lane == 0) { out[0] = s0 * inv_p; out[1] = s1 * inv_f; }
}

// corner [B,F,3,3]: d (gout . out) / d (corner k of face f); wp = 2 / (B P), wf = 2 / (B F)
__global__ __launch_bounds__(PM_SCAN) void pointmesh_bwd_face_kernel(const float* __restrict__ gout, const float* __restrict__ points,
                                                                 const float* __restrict__ verts, const int* __restrict__ faces,
                                                                 const int* __restrict__ face_of_point,
                                                                 const int* __restrict__ point_of_face, int P, int V, int F,
                                                                 float wp, float wf, float* __restrict__ corner) {
    const int f = blockIdx.x * PM_SCAN + threadIdx.x, b = blockIdx.y;
    const bool live = f < F;
    const float* pts = points + (long long)b * P * 3;
    const int* chose = face_of_point + (long long)b * P;
    const float cp = gout[0] * wp, cf = gout[1] * wf;
    PmFace T = PmFace{};
    float g0x = 0.0f, g0y = 0.0f, g0z = 0.0f, g1x = 0.0f, g1y = 0.0f, g1z = 0.0f, g2x = 0.0f, g2y = 0.0f, g2z = 0.0f;
    if (live) {
        T = pm_face_of(verts + (long long)b * V * 3, faces, f);
        const PmHit h = pm_closest(T, pm_ld(pts, point_of_face[(long long)b * F + f]));
        const float k0 = -cf * (1.0f - h.w1 - h.w2), k1 = -cf * h.w1, k2 = -cf * h.w2;
        g0x = k0 * h.rx; g0y = k0 * h.ry; g0z = k0 * h.rz;
        g1x = k1 * h.rx; g1y = k1 * h.ry; g1z = k1 * h.rz;
        g2x = k2 * h.rx; g2y = k2 * h.ry; g2z = k2 * h.rz;
    }
    // an index of a face past the end never occurs in the list, so such a work-item adds nothing and needs no guard
    auto add = [&](int k) {
        const PmHit h = pm_closest(T, pm_ld(pts, k));
        const float k0 = -cp * (1.0f - h.w1 - h.w2), k1 = -cp * h.w1, k2 = -cp * h.w2;
        g0x = fmaf(k0, h.rx, g0x); g0y = fmaf(k0, h.ry, g0y); g0z = fmaf(k0, h.rz, g0z);
        g1x = fmaf(k1, h.rx, g1x); g1y = fmaf(k1, h.ry, g1y); g1z = fmaf(k1, h.rz, g1z);
        g2x = fmaf(k2, h.rx, g2x); g2y = fmaf(k2, h.ry, g2y); g2z = fmaf(k2, h.rz, g2z);
    };
    int k = 0;
    for (; k + PM_BATCH <= P; k += PM_BATCH) {                  // uniform addresses: PM_BATCH scalar loads in flight at once
        int idx[PM_BATCH];
#pragma unroll
        for (int u = 0; u < PM_BATCH; ++u) idx[u] = chose[k + u];
#pragma unroll
        for (int u = 0; u < PM_BATCH; ++u) if (idx[u] == f) add(k + u);
    }
    for (; k < P; ++k) if (chose[k] == f) add(k);
    if (live) {
        float* o = corner + ((long long)b * F + f) * 9;
        st3(o, g0x, g0y, g0z); st3(o + 3, g1x, g1y, g1z); st3(o + 6, g2x, g2y, g2z);
    }
}

__global__ __launch_bounds__(PM_SCAN) void pointmesh_bwd_point_kernel(const float* __restrict__ gout, const float* __restrict__ points,
                                                                  const float* __restrict__ verts, const int* __restrict__ faces,
                                                                  const int* __restrict__ face_of_point,
                                                                  const int* __restrict__ point_of_face, int P, int V, int F,
                                                                  float wp, float wf, float* __restrict__ dpoints) {
    const int i = blockIdx.x * PM_SCAN + threadIdx.x, b = blockIdx.y;
    const bool live = i < P;
    const float* v = verts + (long long)b * V * 3;
    const int* chose = point_of_face + (long long)b * F;
    const float cp = gout[0] * wp, cf = gout[1] * wf;
    PmVec p = PmVec{0.0f, 0.0f, 0.0f};
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (live) {
        p = pm_ld(points, (long long)b * P + i);
        const PmHit h = pm_closest(pm_face_of(v, faces, face_of_point[(long long)b * P + i]), p);
        gx = cp * h.rx; gy = cp * h.ry; gz = cp * h.rz;
    }
    auto add = [&](int k) {
        const PmHit h = pm_closest(pm_face_of(v, faces, k), p);
        gx = fmaf(cf, h.rx, gx); gy = fmaf(cf, h.ry, gy); gz = fmaf(cf, h.rz, gz);
    };
    int k = 0;
    for (; k + PM_BATCH <= F; k += PM_BATCH) {
        int idx[PM_BATCH];
#pragma unroll
        for (int u = 0; u < PM_BATCH; ++u) idx[u] = chose[k + u];
#pragma unroll
        for (int u = 0; u < PM_BATCH; ++u) if (idx[u] == i) add(k + u);
    }
    for (; k < F; ++k) if (chose[k] == i) add(k);
    if (live) st3(dpoints + ((long long)b * P + i) * 3, gx, gy, gz);
}

__global__ __launch_bounds__(PM_GATHER_BLOCK) void pointmesh_bwd_gather_kernel(const float* __restrict__ corner,
                                                                              const int* __restrict__ vf_ptr,
                                                                              const int* __restrict__ vf, int V, int F,
                                                                              float* __restrict__ dverts) {
    const int k = blockIdx.x * PM_GATHER_BLOCK + threadIdx.x, b = blockIdx.y;
    if (k >= V) return;
    const float* c = corner + (long long)b * F * 9;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    const int x1 = vf_ptr[k + 1];
    for (int x = vf_ptr[k]; x < x1; ++x) {
        const F3 g = ld3(c + (long long)(vf[x] >> 2) * 9 + (vf[x] & 3) * 3);
        gx += g.x; gy += g.y; gz += g.z;
    }
    st3(dverts + ((long long)b * V + k) * 3, gx, gy, gz);
}

}  // namespace vpn

using namespace vpn;

static int pointmesh_check(int B, int P, int V, int F) {
    if (B <= 0 || P <= 0 || V <= 0 || F <= 0) return VPN_E_BADARG;
    if (B > 65535 || P > VPN_POINTMESH_MAX_ITEMS || V > VPN_POINTMESH_MAX_ITEMS || F > VPN_POINTMESH_MAX_ITEMS) return VPN_E_TOOBIG;
    return 0;
}

// the grid of the pair scan: point tiles, face slices and faces per slice.  About 1024 workgroups (four to a CU) when the
// faces allow it, a slice never under VPN_POINTMESH_MIN_SLICE faces nor more than VPN_POINTMESH_MAX_SLICES slices; from the
// shape alone, so the same shape always reduces in the same order.
struct PmPlan { int tiles, slices, slice_faces, chunks; };
static PmPlan pointmesh_plan(int B, int P, int F) {
    PmPlan pl;
    pl.tiles = (P + PM_TILE - 1) / PM_TILE;
    const long long groups = (long long)B * pl.tiles;
    long long want = (1024 + groups - 1) / groups;
    long long cap = (F + VPN_POINTMESH_MIN_SLICE - 1) / VPN_POINTMESH_MIN_SLICE;
    if (cap > VPN_POINTMESH_MAX_SLICES) cap = VPN_POINTMESH_MAX_SLICES;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    pl.slice_faces = (int)((F + want - 1) / want);
    pl.slices = (F + pl.slice_faces - 1) / pl.slice_faces;
    pl.chunks = ((P > F ? P : F) + PM_TILE - 1) / PM_TILE;
    return pl;
}

// the workspace in 4-byte words: face records, the partial minima of both directions, the chunk sums.  The backward's
// corner gradients [B,F,9] lie where the records were.
struct PmLayout { size_t rec, pp, pf, sums, total; };
static PmLayout pointmesh_layout(int B, int P, int F, const PmPlan& pl) {
    PmLayout L;
    L.rec = 0;
    L.pp = L.rec + (size_t)B * F * 16;
    L.pf = L.pp + (size_t)B * pl.slices * P * 2;
    L.sums = L.pf + (size_t)B * pl.tiles * F * 2;
    L.total = L.sums + (size_t)B * pl.chunks * 2;
    return L;
}

extern "C" size_t vpn_pointmesh_workspace(int B, int P, int V, int F) {
    if (pointmesh_check(B, P, V, F)) return 0;
    return pointmesh_layout(B, P, F, pointmesh_plan(B, P, F)).total * 4;
}

extern "C" int vpn_pointmesh_fwd(const float* points, const float* verts, const int32_t* faces, int B, int P, int V, int F,
                                 void* workspace, size_t workspace_bytes, float* dist_p, int32_t* face_of_point, float* dist_f,
                                 int32_t* point_of_face, float* out, void* stream) {
    if (!points || !verts || !faces || !workspace) return VPN_E_BADARG;
    const int rc = pointmesh_check(B, P, V, F);
    if (rc) return rc;
    const PmPlan pl = pointmesh_plan(B, P, F);
    const PmLayout L = pointmesh_layout(B, P, F, pl);
    if (workspace_bytes < L.total * 4) return VPN_E_BADARG;
    float* ws = (float*)workspace;
    PmFace* rec = (PmFace*)(ws + L.rec);
    float* pp_d = ws + L.pp;
    int* pp_i = (int*)(pp_d + (size_t)B * pl.slices * P);
    float* pf_d = ws + L.pf;
    int* pf_i = (int*)(pf_d + (size_t)B * pl.tiles * F);
    float* sums = ws + L.sums;
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(pointmesh_prep_kernel, dim3((F + 255) / 256, B), dim3(256), 0, s, verts, (const int*)faces, V, F, rec);
    VPN_LAUNCH(pointmesh_pair_kernel, dim3(pl.tiles, pl.slices, B), dim3(256), 0, s, points, (const PmFace*)rec, P, F, pl.tiles,
               pl.slices, pl.slice_faces, pp_d, pp_i, pf_d, pf_i);
    VPN_LAUNCH(pointmesh_merge_kernel, dim3(pl.chunks, B), dim3(256), 0, s, (const float*)pp_d, (const int*)pp_i,
               (const float*)pf_d, (const int*)pf_i, P, F, pl.tiles, pl.slices, pl.chunks, dist_p, (int*)face_of_point, dist_f,
               (int*)point_of_face, sums);
    if (out)
        VPN_LAUNCH(pointmesh_final_kernel, dim3(1), dim3(64), 0, s, (const float*)sums, B * pl.chunks,
                   (float)(1.0 / ((double)B * P)), (float)(1.0 / ((double)B * F)), out);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_pointmesh_bwd(const float* grad, const float* points, const float* verts, const int32_t* faces,
                                 const int32_t* face_of_point, const int32_t* point_of_face, const int32_t* vf_ptr,
                                 const int32_t* vf, int B, int P, int V, int F, void* workspace, size_t workspace_bytes,
                                 float* dpoints, float* dverts, void* stream) {
    if (!grad || !points || !verts || !faces || !face_of_point || !point_of_face) return VPN_E_BADARG;
    if (dverts && (!vf_ptr || !vf || !workspace)) return VPN_E_BADARG;
    const int rc = pointmesh_check(B, P, V, F);
    if (rc) return rc;
    if (dverts && workspace_bytes < (size_t)B * F * 9 * 4) return VPN_E_BADARG;
    const float wp = (float)(2.0 / ((double)B * P)), wf = (float)(2.0 / ((double)B * F));
    hipStream_t s = (hipStream_t)stream;
    if (dverts) {
        float* corner = (float*)workspace;
        VPN_LAUNCH(pointmesh_bwd_face_kernel, dim3((F + PM_SCAN - 1) / PM_SCAN, B), dim3(PM_SCAN), 0, s, grad, points, verts,
                   (const int*)faces, (const int*)face_of_point, (const int*)point_of_face, P, V, F, wp, wf, corner);
        VPN_LAUNCH(pointmesh_bwd_gather_kernel, dim3((V + PM_GATHER_BLOCK - 1) / PM_GATHER_BLOCK, B), dim3(PM_GATHER_BLOCK), 0, s,
                   (const float*)corner, (const int*)vf_ptr, (const int*)vf, V, F, dverts);
    }
    if (dpoints)
        VPN_LAUNCH(pointmesh_bwd_point_kernel, dim3((P + PM_SCAN - 1) / PM_SCAN, B), dim3(PM_SCAN), 0, s, grad, points, verts,
                   (const int*)faces, (const int*)face_of_point, (const int*)point_of_face, P, V, F, wp, wf, dpoints);
    VPN_LAUNCH_CHECK();
    return 0;
}
