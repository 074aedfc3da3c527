// occupancy.hip — volumetric evaluation: "is x inside" for the two things this project predicts and compares
// with, and the intersection over union of two occupancies per sample with the per-class bookkeeping of an epoch.
//
//   occ_prims_kernel       one work-item per (query, sample): x~ = R^T (x - t) / v per primitive, inside iff x~.x~ <= 1 (sphere)
//                          or every |x~_i| <= 1 (cuboid); the K pose records are staged in LDS once per workgroup, OC_STAGE at a
//                          time, by the lanes of the workgroup (make_pose, the sampler's and the raster's own function).
//   winding_prep_kernel    one work-item per (face, sample): the record of the face (OcFace, 12 words: the three corners after the
//                          affine map, and whether the face counts: 0 a vertex index outside its mesh or no area (e1 x e2 =
//                          (0,0,0)), 1 yes, 2 a corner that is not finite).
//   winding_kernel         one workgroup per (tile of 256 queries, slice of the faces, sample).  A work-item keeps its query in
//                          registers and walks the records of the slice; the record index is uniform, so the records come through
//                          scalar loads and cost no LDS.  Per pair the signed solid angle by Van Oosterom and Strackee, 2 atan2(a .
//                          (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), exactly 0 where the numerator is 0; the terms of
//                          a slice are added in ascending face order in fp64.  Out: partial sums [B,slices,Q] fp64.
//   winding_merge_kernel   one work-item per (query, sample): the partial sums in ascending slice order, over 4 pi in fp64,
//                          rounded to fp32 once; NaN for a query that is not finite; occ = w > 0.5 on the rounded value.
//   voliou_sample_kernel   one workgroup per sample: the four integer counts (and, or, prediction, ground truth) and the row of
//                          W = 5 values formed from them in fp64.
//   voliou_book_kernel     ONE workgroup, launched after the sample kernel on the same stream: state += the batch.
//
// No atomics, no scratch, no hand-off between workgroups, nothing allocated: every sum has one fixed order, so the results are
// bit-equal from run to run, and a query set shared by the batch is read through a sample stride of 0 by the same code.
//
// State (vpn_voliou_state_size), zeroed by the caller, W = 5:
//   doubles  total[W]  class_sum[C][W]          int64  n_samples  n_batches  n_empty  n_invalid  class_n[C]
//
// Built with -ffp-contract=off: every product and sum below is rounded by itself, as tests/occupancy_ref.py states them; a
// face whose three corners coincide then has a numerator of exactly 0 whatever the query is.
#include "vpn_common.h"
#include "occupancy_prim.h"
#include <float.h>

namespace {

constexpr int OC_TILE = VPN_OCCUPANCY_TILE;          // queries per workgroup
using vpn::OC_STAGE;                                 // primitives staged in LDS at a time: one per lane (occupancy_prim.h)
using vpn::OcPrim;
constexpr int OC_W = VPN_VOLIOU_WIDTH;               // iou precision recall vol_pred vol_gt
constexpr int OC_CHUNK = 256;                        // samples of a batch the bookkeeping stages in LDS at a time
constexpr int OC_MAX_ITEMS = VPN_OCCUPANCY_MAX_ITEMS;    // Q, P, F, C

struct __attribute__((aligned(16))) OcFace { float ax, ay, az, bx, by, bz, cx, cy, cz; int live, pad0, pad1; };
static_assert(sizeof(OcFace) == 48, "a face record is 12 words");

inline size_t oc_doubles(int C) { return (1 + (size_t)C) * OC_W; }
inline size_t oc_counts(int C) { return 4 + (size_t)C; }

__device__ inline bool oc_finite(float x) { return fabsf(x) <= FLT_MAX; }          // false for inf and NaN

// the affine rows of view_center_xforms / genre_xforms, summed the way surfeval_normals_kernel maps its corners
__device__ inline vpn::F3 oc_map(const float* __restrict__ m, vpn::F3 v) {
    return vpn::F3{m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3], m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7],
                   m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11]};
}

// queries [Q,3] (q_stride 0) or [B,Q,3] (q_stride 3 Q); occ [B,Q] and owner [B,Q] may each be NULL
__global__ __launch_bounds__(256) void occ_prims_kernel(const float* __restrict__ params, const int32_t* __restrict__ kinds,
                                                        const float* __restrict__ queries, long long q_stride, int K, int Q,
                                                        uint8_t* __restrict__ occ, int32_t* __restrict__ owner) {
    __shared__ OcPrim s_p[OC_STAGE];
    const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.x * OC_TILE + tid;
    const bool valid = i < Q;
    const vpn::F3 x = valid ? vpn::ld3(queries + (size_t)b * q_stride + (size_t)i * 3) : vpn::F3{0.0f, 0.0f, 0.0f};
    int own = -1;
    for (int base = 0; base < K; base += OC_STAGE) {
        const int m = min(OC_STAGE, K - base);
        __syncthreads();                                 // the previous records have been read
        if (tid < m) vpn::oc_stage_prim(s_p[tid], params, kinds, b, K, base + tid);
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const OcPrim& p = s_p[k];                    // the same address for every lane: an LDS broadcast
            const vpn::F3 y = vpn::oc_local(p, x);
            const float y0 = y.x, y1 = y.y, y2 = y.z;
            // a NaN fails every comparison: outside
            const bool in = p.sphere ? (y0 * y0 + y1 * y1 + y2 * y2 <= 1.0f)
                                     : (fabsf(y0) <= 1.0f && fabsf(y1) <= 1.0f && fabsf(y2) <= 1.0f);
            if (in && own < 0) own = base + k;
        }
    }
    if (valid) {
        const size_t o = (size_t)b * Q + i;
        if (occ) occ[o] = own >= 0;
        if (owner) owner[o] = own;
    }
}

// the vertices and faces sample b reads: batched (vert_offset == NULL) verts [B,P,3] and ONE faces [F,3]; ragged verts [P,3],
// faces [F,3] mesh-local, sample b is mesh b.  A table entry that does not describe the packed arrays names nothing.
struct OcMesh { long long vbase, nv, fbase, nf; };
__device__ inline OcMesh oc_mesh(const int32_t* __restrict__ vert_offset, const int32_t* __restrict__ face_offset, int b, int P,
                                 int F) {
    OcMesh m;
    if (face_offset) {
        m.fbase = face_offset[b]; m.nf = (long long)face_offset[b + 1] - m.fbase;
        if (m.fbase < 0 || m.nf < 0 || m.fbase + m.nf > F) { m.fbase = 0; m.nf = 0; }
        m.vbase = 0; m.nv = 0;
        if (vert_offset) {
            m.vbase = vert_offset[b]; m.nv = (long long)vert_offset[b + 1] - m.vbase;
            if (m.vbase < 0 || m.nv < 0 || m.vbase + m.nv > P) { m.vbase = 0; m.nv = 0; }
        }
    } else {
        m.vbase = (long long)b * P; m.nv = P; m.fbase = 0; m.nf = F;
    }
    return m;
}

// rec: batched [B,F], ragged [F] (the packed faces; every mesh belongs to one sample).  `stride` work-items walk a mesh.
__global__ __launch_bounds__(256) void winding_prep_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                           const int32_t* __restrict__ vert_offset,
                                                           const int32_t* __restrict__ face_offset, const float* __restrict__ xforms,
                                                           int P, int F, int stride, OcFace* __restrict__ rec) {
    const int b = blockIdx.y;
    const OcMesh me = oc_mesh(vert_offset, face_offset, b, P, F);
    OcFace* out = rec + (face_offset ? me.fbase : (long long)b * F);
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < me.nf; f += stride) {
        const int32_t* fc = faces + (size_t)(me.fbase + f) * 3;
        const long long i0 = fc[0], i1 = fc[1], i2 = fc[2];
        OcFace T = OcFace{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0};
        if (i0 >= 0 && i0 < me.nv && i1 >= 0 && i1 < me.nv && i2 >= 0 && i2 < me.nv) {
            vpn::F3 a = vpn::ld3(verts + (size_t)(me.vbase + i0) * 3), p = vpn::ld3(verts + (size_t)(me.vbase + i1) * 3),
                    q = vpn::ld3(verts + (size_t)(me.vbase + i2) * 3);
            if (xforms) {
                const float* m = xforms + (size_t)b * 12;
                a = oc_map(m, a); p = oc_map(m, p); q = oc_map(m, q);
            }
            const bool fin = oc_finite(a.x) && oc_finite(a.y) && oc_finite(a.z) && oc_finite(p.x) && oc_finite(p.y) &&
                             oc_finite(p.z) && oc_finite(q.x) && oc_finite(q.y) && oc_finite(q.z);
            // e1 x e2 = (0,0,0): a face of no area counts for nothing, whatever the query's roundings make of a . (b x c)
            const float e1x = p.x - a.x, e1y = p.y - a.y, e1z = p.z - a.z, e2x = q.x - a.x, e2y = q.y - a.y, e2z = q.z - a.z;
            const bool flat = e1y * e2z - e1z * e2y == 0.0f && e1z * e2x - e1x * e2z == 0.0f && e1x * e2y - e1y * e2x == 0.0f;
            T = OcFace{a.x, a.y, a.z, p.x, p.y, p.z, q.x, q.y, q.z, !fin ? 2 : (flat ? 0 : 1), 0, 0};
        }
        out[f] = T;
    }
}

// 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) of the corners seen from x; 0 where the numerator is 0
__device__ inline float oc_solid_angle(const OcFace& T, vpn::F3 x) {
    const float ax = T.ax - x.x, ay = T.ay - x.y, az = T.az - x.z;
    const float bx = T.bx - x.x, by = T.by - x.y, bz = T.bz - x.z;
    const float cx = T.cx - x.x, cy = T.cy - x.y, cz = T.cz - x.z;
    const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz),
                lc = sqrtf(cx * cx + cy * cy + cz * cz);
    const float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
    const float num = ax * nx + ay * ny + az * nz;
    const float ab = ax * bx + ay * by + az * bz, bc = bx * cx + by * cy + bz * cz, ca = cx * ax + cy * ay + cz * az;
    const float den = la * lb * lc + ab * lc + bc * la + ca * lb;
    return num == 0.0f ? 0.0f : 2.0f * atan2f(num, den);
}

__global__ __launch_bounds__(256) void winding_kernel(const float* __restrict__ queries, long long q_stride,
                                                      const OcFace* __restrict__ rec, const int32_t* __restrict__ face_offset,
                                                      int Q, int F, int slices, int slice_faces, double* __restrict__ part) {
    const int tid = threadIdx.x, tile = blockIdx.x, sl = blockIdx.y, b = blockIdx.z;
    const int i = tile * OC_TILE + tid;
    const bool valid = i < Q;
    const vpn::F3 x = valid ? vpn::ld3(queries + (size_t)b * q_stride + (size_t)i * 3) : vpn::F3{0.0f, 0.0f, 0.0f};
    const OcMesh me = oc_mesh(nullptr, face_offset, b, 0, F);
    const OcFace* r = rec + (face_offset ? me.fbase : (long long)b * F);
    // slice sl of the mesh's faces; the last slice runs to the end, so no face is left out when a mesh has more faces than
    // the plan was made for
    const long long f0 = min((long long)sl * slice_faces, me.nf);
    const long long f1 = sl == slices - 1 ? me.nf : min(f0 + slice_faces, me.nf);
    double acc = 0.0;
    for (long long f = f0; f < f1; ++f) {
        const OcFace T = r[f];                                                 // uniform index: scalar loads
        if (T.live == 0) continue;
        acc += T.live == 1 ? (double)oc_solid_angle(T, x) : (double)NAN;
    }
    if (valid) part[((size_t)b * slices + sl) * Q + i] = acc;
}

__global__ __launch_bounds__(256) void winding_merge_kernel(const double* __restrict__ part, const float* __restrict__ queries,
                                                            long long q_stride, int Q, int slices, float* __restrict__ w,
                                                            uint8_t* __restrict__ occ) {
    const int b = blockIdx.y, i = blockIdx.x * OC_TILE + threadIdx.x;
    if (i >= Q) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += part[((size_t)b * slices + k) * Q + i];
    const vpn::F3 x = vpn::ld3(queries + (size_t)b * q_stride + (size_t)i * 3);
    float v = (float)(s / 12.566370614359172);                                 // 4 pi
    if (!(oc_finite(x.x) && oc_finite(x.y) && oc_finite(x.z))) v = NAN;
    const size_t o = (size_t)b * Q + i;
    if (w) w[o] = v;
    if (occ) occ[o] = v > 0.5f;                                                // NaN is outside
}

// One workgroup (256 lanes) per sample.  Lane t owns elements t, t + 256, ...; xor tree over the wave; the four waves in
// order.  Counts are integers and exact; the five quotients are formed in fp64 from them and rounded once.
__global__ __launch_bounds__(256) void voliou_sample_kernel(const uint8_t* __restrict__ occ_pred, const uint8_t* __restrict__ occ_gt,
                                                            int Q, float* __restrict__ rows, int32_t* __restrict__ counts) {
    __shared__ int cred[4][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* p = occ_pred + (size_t)b * Q;
    const uint8_t* g = occ_gt + (size_t)b * Q;
    int c[4] = {0, 0, 0, 0};                                   // and, or, prediction, ground truth
    for (int i = tid; i < Q; i += 256) {
        const int a = p[i] != 0, d = g[i] != 0;
        c[0] += a & d; c[1] += a | d; c[2] += a; c[3] += d;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cred[wave][k] = c[k];
    }
    __syncthreads();
    if (tid < 4) counts[(size_t)b * 4 + tid] = (cred[0][tid] + cred[1][tid]) + (cred[2][tid] + cred[3][tid]);
    if (tid >= 64 && tid < 64 + OC_W) {
        const int k = tid - 64;
        const int jn = k < 3 ? 0 : k - 1, jd = k < 3 ? k + 1 : 0;             // which count is the numerator, the denominator
        const int num = (cred[0][jn] + cred[1][jn]) + (cred[2][jn] + cred[3][jn]);
        const int den = k < 3 ? (cred[0][jd] + cred[1][jd]) + (cred[2][jd] + cred[3][jd]) : Q;
        rows[(size_t)b * OC_W + k] = den ? (float)((double)num / (double)den) : 0.0f;
    }
}

// ONE workgroup.  Work-item j < (1 + C) W owns (group j / W, column j % W), strided by 256: group 0 is the total over ALL
// samples, group 1 + c is class c.  It walks the samples in order b = 0 .. B-1, which is the order Python's `+= float(x)`
// adds in, so the state is bit-equal to a host loop over the rows.  Lane c owns class_n[c]; lane 255 the four counts.
__global__ __launch_bounds__(256) void voliou_book_kernel(const float* __restrict__ rows, const int32_t* __restrict__ counts_in,
                                                          const int32_t* __restrict__ class_index, int B, int C,
                                                          double* __restrict__ state) {
    __shared__ float s_row[OC_CHUNK * OC_W];
    __shared__ int s_cls[OC_CHUNK];
    __shared__ int s_union[OC_CHUNK];
    const int tid = threadIdx.x;
    const int items = (1 + C) * OC_W;
    long long* counts = reinterpret_cast<long long*>(state + (size_t)items);
    long long invalid = 0, empty = 0;
    for (int base = 0; base < B; base += OC_CHUNK) {
        const int m = min(OC_CHUNK, B - base);
        __syncthreads();                                 // the previous chunk has been read
        for (int i = tid; i < m * OC_W; i += 256) s_row[i] = rows[(size_t)base * OC_W + i];
        for (int i = tid; i < m; i += 256) { s_cls[i] = class_index[base + i]; s_union[i] = counts_in[(size_t)(base + i) * 4 + 1]; }
        __syncthreads();
        for (int j = tid; j < items; j += 256) {
            const int g = j / OC_W, k = j - g * OC_W;
            double a = state[j];
            for (int i = 0; i < m; ++i) {
                if (g == 0 || s_cls[i] == g - 1) a += (double)s_row[i * OC_W + k];
            }
            state[j] = a;
        }
        for (int c = tid; c < C; c += 256) {
            long long k = counts[4 + c];
            for (int i = 0; i < m; ++i) k += s_cls[i] == c;
            counts[4 + c] = k;
        }
        if (tid == 255) {
            for (int i = 0; i < m; ++i) { invalid += (unsigned)s_cls[i] >= (unsigned)C; empty += s_union[i] == 0; }
        }
    }
    if (tid == 255) {
        counts[0] += B;
        counts[1] += 1;
        counts[2] += empty;
        counts[3] += invalid;
    }
}

// the grid of the winding scan: query tiles, face slices and faces per slice.  About 1024 workgroups (four to a CU) when the
// faces allow it, a slice never under VPN_WINDING_MIN_SLICE faces nor more than VPN_WINDING_MAX_SLICES slices; from the shape
// alone, so the same shape always adds in the same order.
struct OcPlan { int tiles, slices, slice_faces; };
OcPlan winding_plan(int B, int Q, int max_faces) {
    OcPlan pl;
    pl.tiles = (Q + OC_TILE - 1) / OC_TILE;
    const long long groups = (long long)B * pl.tiles;
    long long want = (1024 + groups - 1) / groups;
    long long cap = (max_faces + VPN_WINDING_MIN_SLICE - 1) / VPN_WINDING_MIN_SLICE;
    if (cap > VPN_WINDING_MAX_SLICES) cap = VPN_WINDING_MAX_SLICES;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    pl.slice_faces = (int)((max_faces + want - 1) / want);
    pl.slices = (max_faces + pl.slice_faces - 1) / pl.slice_faces;
    return pl;
}

// the workspace in bytes: the partial sums (fp64), then the face records (16-byte aligned)
struct OcLayout { size_t part, rec, total; };
OcLayout winding_layout(int B, int Q, int F, bool ragged, const OcPlan& pl) {
    OcLayout L;
    L.part = 0;
    L.rec = ((size_t)B * pl.slices * Q * 8 + 15) & ~(size_t)15;
    L.total = L.rec + (ragged ? (size_t)F : (size_t)B * F) * sizeof(OcFace);
    return L;
}

int winding_check(int B, int Q, int F, int ragged, int& max_faces) {
    if (B <= 0 || Q <= 0 || F <= 0) return VPN_E_BADARG;
    if (!ragged) max_faces = F;
    if (max_faces <= 0 || max_faces > F) return VPN_E_BADARG;
    if (B > 65535 || Q > OC_MAX_ITEMS || F > OC_MAX_ITEMS) return VPN_E_TOOBIG;
    return 0;
}

}  // namespace

extern "C" int vpn_occupancy_prims(const float* params, const int32_t* kinds, const float* queries, int shared_queries, int B, int K,
                                   int Q, uint8_t* occ, int32_t* owner, void* stream) {
    if (!params || !kinds || !queries || (!occ && !owner)) return VPN_E_BADARG;
    if (B <= 0 || K <= 0 || Q <= 0) return VPN_E_BADARG;
    if (B > 65535 || Q > OC_MAX_ITEMS || K > VPN_MAX_PRIMS) return VPN_E_TOOBIG;
    VPN_LAUNCH(occ_prims_kernel, dim3((Q + OC_TILE - 1) / OC_TILE, B), dim3(256), 0, (hipStream_t)stream, params, kinds, queries,
               shared_queries ? 0LL : 3LL * Q, K, Q, occ, owner);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_winding_plan(int B, int Q, int max_faces, int* slice_faces) {
    int mf = max_faces;
    const int rc = winding_check(B, Q, max_faces, 0, mf);
    if (rc) return rc;
    const OcPlan pl = winding_plan(B, Q, max_faces);
    if (slice_faces) *slice_faces = pl.slice_faces;
    return pl.slices;
}

extern "C" size_t vpn_winding_workspace(int B, int Q, int F, int ragged, int max_faces) {
    if (winding_check(B, Q, F, ragged, max_faces)) return 0;
    return winding_layout(B, Q, F, ragged != 0, winding_plan(B, Q, max_faces)).total;
}

extern "C" int vpn_winding_number(const float* verts, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                                  const float* xforms, const float* queries, int shared_queries, int B, int Q, int P, int F,
                                  int max_faces, void* workspace, size_t workspace_bytes, float* w, uint8_t* occ, void* stream) {
    if (!verts || !faces || !queries || !workspace || (!w && !occ)) return VPN_E_BADARG;
    if ((vert_offset == nullptr) != (face_offset == nullptr)) return VPN_E_BADARG;
    if (P <= 0) return VPN_E_BADARG;
    const bool ragged = face_offset != nullptr;
    const int rc = winding_check(B, Q, F, ragged, max_faces);
    if (rc) return rc;
    if (P > OC_MAX_ITEMS) return VPN_E_TOOBIG;
    const OcPlan pl = winding_plan(B, Q, max_faces);
    const OcLayout L = winding_layout(B, Q, F, ragged, pl);
    if (workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(workspace) & 15)) return VPN_E_BADARG;
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + L.part);
    OcFace* rec = reinterpret_cast<OcFace*>(static_cast<char*>(workspace) + L.rec);
    const long long q_stride = shared_queries ? 0LL : 3LL * Q;
    const int prep_groups = (max_faces + 255) / 256;
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(winding_prep_kernel, dim3(prep_groups, B), dim3(256), 0, s, verts, faces, vert_offset, face_offset, xforms, P, F,
               prep_groups * 256, rec);
    VPN_LAUNCH(winding_kernel, dim3(pl.tiles, pl.slices, B), dim3(256), 0, s, queries, q_stride, (const OcFace*)rec, face_offset, Q,
               F, pl.slices, pl.slice_faces, part);
    VPN_LAUNCH(winding_merge_kernel, dim3(pl.tiles, B), dim3(256), 0, s, (const double*)part, queries, q_stride, Q, pl.slices, w,
               occ);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vpn_voliou_state_size(int num_classes) {
    if (num_classes <= 0 || num_classes > OC_MAX_ITEMS) return 0;
    return (oc_doubles(num_classes) + oc_counts(num_classes)) * 8;
}

extern "C" int vpn_voliou_accumulate(const uint8_t* occ_pred, const uint8_t* occ_gt, const int32_t* class_index, int B, int Q,
                                     int num_classes, void* state, float* rows, int32_t* counts, void* stream) {
    if (!occ_pred || !occ_gt || !class_index || !state || !rows || !counts) return VPN_E_BADARG;
    if (B <= 0 || Q <= 0 || num_classes <= 0) return VPN_E_BADARG;
    if (reinterpret_cast<uintptr_t>(state) & 7) return VPN_E_BADARG;
    if (B > 65535 || Q > OC_MAX_ITEMS || num_classes > OC_MAX_ITEMS) return VPN_E_TOOBIG;
    VPN_LAUNCH(voliou_sample_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, occ_pred, occ_gt, Q, rows, counts);
    VPN_LAUNCH_CHECK();
    VPN_LAUNCH(voliou_book_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)rows, (const int32_t*)counts, class_index,
               B, num_classes, static_cast<double*>(state));
    VPN_LAUNCH_CHECK();
    return 0;
}
