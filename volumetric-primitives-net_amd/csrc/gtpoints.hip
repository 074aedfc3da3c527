// gtpoints.hip — the ground-truth stage (gfx950): area-weighted surface samples of a RAGGED batch of triangle meshes.
//
// Replaces (reference file:line) ShapeNetDataset._load_sample_points (modules/dataset/dataset.py:161-165:
// TriangleMesh.from_obj(p).sample(2048), called twice per item, dataset.py:42-43) and GenReDataset._load_points
// (modules/dataset/genre.py:66-74) for a whole batch of S meshes of DIFFERENT sizes: T point sets per mesh come out of ONE
// cumulative-area table per mesh (the view-centred mesh of dataset.py:168-184 is the canonical one under an affine map, so
// its table is the canonical table times a constant: the same faces are chosen).  kaolin is absent: the result is defined
// by DESIGN.md 4.15 and restated by tests/gtpoints_ref.py (parity with kaolin unpinned, like mesh.hip).
//
// Three launches per batch, whatever S is, and none of them walks a mesh's face list in one workgroup:
//   1. ragged_chunk_kernel   one workgroup per CHUNK of the packed face list (a chunk never straddles two meshes): face
//                            areas, their inclusive fp64 prefix sums inside the chunk, the chunk's total;
//   2. ragged_base_kernel    one wave per mesh: the running sum of its chunks' totals (a few hundred values for a
//                            400 k-face mesh), in place, and the mesh's total area in fp32;
//   3. ragged_sample_kernel  one lane per (mesh, set, point): Philox draw, binary search over the mesh's chunks, binary
//                            search inside the chunk, gather of the three corners, barycentric point, affine map.
// Every fp64 sum below is associated so that the table (chunk base + in-chunk prefix, rounded to fp32) is non-decreasing
// in the face index BY CONSTRUCTION (x + y is monotone in y under round-to-nearest); the two-level search therefore picks
// the face a flat search over the rounded table would pick.  Compiled with -ffp-contract=off: every
// product and sum is rounded by itself.
#include "vpn_common.h"

namespace vpn {

constexpr int RS_CHUNK = VPN_RAGGED_CHUNK;
constexpr int RS_BLOCK = 256;
constexpr int RS_PER = RS_CHUNK / RS_BLOCK;              // consecutive faces of one lane
static_assert(RS_PER * RS_BLOCK == RS_CHUNK && RS_BLOCK % 64 == 0, "a chunk is RS_PER faces for each of RS_BLOCK lanes");

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The packed arrays are data: every offset read from them is clamped into its array before it is used, so that a bad
// table can neither fault nor reach beyond the buffers.
struct MeshView { const float* v; int P; };
__device__ inline MeshView mesh_view(const float* __restrict__ verts, const int32_t* __restrict__ vert_offset, int s, int sumP) {
    const int v0 = clampi(vert_offset[s], 0, sumP - 1);
    return MeshView{verts + (size_t)v0 * 3, clampi(vert_offset[s + 1] - v0, 1, sumP - v0)};
}
struct ChunkView { int mesh, f0, cnt; };
__device__ inline ChunkView chunk_view(const int32_t* __restrict__ chunks, int c, int S, int sumF) {
    ChunkView k;
    k.mesh = clampi(chunks[(size_t)c * 3], 0, S - 1);
    k.f0 = clampi(chunks[(size_t)c * 3 + 1], 0, sumF - 1);
    k.cnt = clampi(chunks[(size_t)c * 3 + 2], 1, min(RS_CHUNK, sumF - k.f0));
    return k;
}

struct Tri { F3 a, b, c; };
__device__ inline Tri load_tri(const MeshView& M, const int32_t* __restrict__ f) {
    // vertex indices are mesh-local data: clamped to [0, P_s - 1]
    const int ia = clampi(f[0], 0, M.P - 1), ib = clampi(f[1], 0, M.P - 1), ic = clampi(f[2], 0, M.P - 1);
    return Tri{ld3(M.v + (size_t)ia * 3), ld3(M.v + (size_t)ib * 3), ld3(M.v + (size_t)ic * 3)};
}

// inclusive running sum over the 64 lanes of a wave in LANE ORDER (((x0 + x1) + x2) + ...): 64 dependent adds on
// wave-uniform values instead of the 6-step tree of mesh_cdf_kernel, so that lane l + 1 holds exactly (lane l) + x_{l+1}
__device__ inline double wave_running_sum(double x, double carry, int lane) {
    double run = carry, mine = 0.0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        run += __shfl(x, k, 64);
        if (lane == k) mine = run;
    }
    return mine;
}

// ---- 1. areas and in-chunk prefix sums
// local[f] = wave base + (lane prefix + running sum of the lane's own faces up to f), fp64; ctot[c] = the chunk's last entry.
// Faces beyond the chunk's count add +0.0, which is exact: the last lane's last entry is the entry of the last face.
__global__ __launch_bounds__(RS_BLOCK) void ragged_chunk_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                const int32_t* __restrict__ vert_offset,
                                                                const int32_t* __restrict__ chunks, int S, int sumP, int sumF,
                                                                double* __restrict__ local, double* __restrict__ ctot) {
    __shared__ double wtot[RS_BLOCK / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ChunkView K = chunk_view(chunks, c, S, sumF);
    const MeshView M = mesh_view(verts, vert_offset, K.mesh, sumP);
    double inc[RS_PER], run = 0.0;
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        const int i = tid * RS_PER + j;
        double area = 0.0;
        if (i < K.cnt) {
            const Tri t = load_tri(M, faces + (size_t)(K.f0 + i) * 3);
            const float ux = t.b.x - t.a.x, uy = t.b.y - t.a.y, uz = t.b.z - t.a.z;
            const float wx = t.c.x - t.a.x, wy = t.c.y - t.a.y, wz = t.c.z - t.a.z;
            const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            area = (double)(0.5f * sqrtf(nx * nx + ny * ny + nz * nz));
        }
        run += area;
        inc[j] = run;
    }
    const double incl = wave_running_sum(run, 0.0, lane);        // through this lane's faces
    double excl = __shfl_up(incl, 1, 64);                        // before them
    if (lane == 0) excl = 0.0;
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    double base = 0.0;
    for (int w = 0; w < wave; ++w) base += wtot[w];
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        const int i = tid * RS_PER + j;
        const double v = base + (excl + inc[j]);
        if (i < K.cnt) local[(size_t)K.f0 + i] = v;
        if (i == RS_CHUNK - 1) ctot[c] = v;
    }
}

// ---- 2. per mesh: cinc[c] = cinc[c - 1] + ctot[c] over the mesh's chunks, in place and strictly in chunk order (the chunk's
// base is the entry before it), total[s] = the last one rounded to fp32
__global__ __launch_bounds__(RS_BLOCK) void ragged_base_kernel(const int32_t* __restrict__ chunk_offset, int S, int C,
                                                               double* __restrict__ cinc, float* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * (RS_BLOCK / 64) + (threadIdx.x >> 6);
    if (s >= S) return;
    const int c0 = clampi(chunk_offset[s], 0, C - 1), c1 = clampi(chunk_offset[s + 1], c0 + 1, C);
    double carry = 0.0;
    for (int g = c0; g < c1; g += 64) {
        const int c = g + lane;
        const double mine = wave_running_sum(c < c1 ? cinc[c] : 0.0, carry, lane);
        if (c < c1) cinc[c] = mine;
        if (c == c1 - 1) total[s] = (float)mine;
        carry = __shfl(mine, 63, 64);
    }
}

// ---- 3. one lane per (mesh, set, point)
__global__ __launch_bounds__(RS_BLOCK) void ragged_sample_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ vert_offset,
                                                                 const int32_t* __restrict__ face_offset,
                                                                 const int32_t* __restrict__ chunk_offset,
                                                                 const int32_t* __restrict__ chunks, const float* __restrict__ xforms,
                                                                 unsigned xform_mask, const float* __restrict__ u, uint64_t seed,
                                                                 const uint64_t* __restrict__ seed_dev, uint64_t mesh_base, int S, int T,
                                                                 int n, int sumP, int sumF, int C, const double* __restrict__ local,
                                                                 const double* __restrict__ cinc, const float* __restrict__ total,
                                                                 float* __restrict__ points, int32_t* __restrict__ face_idx,
                                                                 float* __restrict__ bary) {
    const int st = blockIdx.y, i = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = st / T, t = st - s * T;
    const size_t o = (size_t)st * n + i;
    float uu[3];
    if (u) { const F3 v = ld3(u + o * 3); uu[0] = v.x; uu[1] = v.y; uu[2] = v.z; }
    else {
        if (seed_dev) seed += *seed_dev;
        philox_uniform3(seed, mesh_base + (uint64_t)s, 0xFFFFFFFFu - (uint32_t)t, (uint32_t)i, uu);
    }
    const int c0 = clampi(chunk_offset[s], 0, C - 1), c1 = clampi(chunk_offset[s + 1], c0 + 1, C);
    const float target = uu[0] * total[s];
    int lo = c0, hi = c1 - 1;                             // first chunk whose last entry exceeds the target, else the last chunk
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((float)cinc[mid] > target) hi = mid; else lo = mid + 1;
    }
    const double base = lo > c0 ? cinc[lo - 1] : 0.0;
    const ChunkView K = chunk_view(chunks, lo, S, sumF);
    const double* lc = local + K.f0;
    int a = 0, b = K.cnt - 1;                             // first face of it whose entry exceeds the target, else its last face
    while (a < b) {
        const int mid = (a + b) >> 1;
        if ((float)(base + lc[mid]) > target) b = mid; else a = mid + 1;
    }
    const int f = K.f0 + a;
    const MeshView M = mesh_view(verts, vert_offset, s, sumP);
    const Tri tr = load_tri(M, faces + (size_t)f * 3);
    const float r = sqrtf(uu[1]);
    const float w0 = 1.0f - r, w1 = r * (1.0f - uu[2]), w2 = r * uu[2];
    float x = w0 * tr.a.x + w1 * tr.b.x + w2 * tr.c.x, y = w0 * tr.a.y + w1 * tr.b.y + w2 * tr.c.y,
          z = w0 * tr.a.z + w1 * tr.b.z + w2 * tr.c.z;
    if (xforms && ((xform_mask >> t) & 1u)) {
        const float* m = xforms + (size_t)st * 12;       // the same 12 values for the whole workgroup: scalar loads
        const float px = x, py = y, pz = z;
        x = m[0] * px + m[1] * py + m[2] * pz + m[3];
        y = m[4] * px + m[5] * py + m[6] * pz + m[7];
        z = m[8] * px + m[9] * py + m[10] * pz + m[11];
    }
    st3(points + o * 3, x, y, z);
    if (face_idx) face_idx[o] = f - clampi(face_offset[s], 0, f);
    if (bary) st3(bary + o * 3, w0, w1, w2);
}

static size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace vpn

using namespace vpn;

extern "C" size_t vpn_ragged_sample_workspace(int sumF, int C, int S) {
    if (sumF <= 0 || C <= 0 || S <= 0) return 0;
    return align16((size_t)sumF * sizeof(double)) + align16((size_t)C * sizeof(double)) + align16((size_t)S * sizeof(float));
}

extern "C" int vpn_ragged_sample(const float* verts, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                                 const int32_t* chunk_offset, const int32_t* chunks, const float* xforms, unsigned xform_mask,
                                 const float* u, uint64_t seed, const uint64_t* seed_dev, uint64_t mesh_base, int S, int T, int n, int sumP, int sumF,
                                 int C, void* workspace, size_t workspace_bytes, float* points, int32_t* face_idx, float* bary,
                                 void* stream) {
    if (!verts || !faces || !vert_offset || !face_offset || !chunk_offset || !chunks || !workspace || !points) return VPN_E_BADARG;
    if (S <= 0 || T <= 0 || n <= 0 || sumP <= 0 || sumF <= 0 || C <= 0) return VPN_E_BADARG;
    if (T > VPN_RAGGED_MAX_SETS || (long long)S * T > 65535 || sumP > 0x7fffffff / 3 || sumF > 0x7fffffff / 3 ||
        n > 0x7fffffff - RS_BLOCK) return VPN_E_TOOBIG;
    if (C > sumF || ((uintptr_t)workspace & 15) != 0 ||
        workspace_bytes < vpn_ragged_sample_workspace(sumF, C, S)) return VPN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    double* local = (double*)workspace;
    double* cinc = (double*)((char*)workspace + align16((size_t)sumF * sizeof(double)));
    float* total = (float*)((char*)cinc + align16((size_t)C * sizeof(double)));
    VPN_LAUNCH(ragged_chunk_kernel, dim3((unsigned)C), dim3(RS_BLOCK), 0, s, verts, faces, vert_offset, chunks, S, sumP, sumF, local, cinc);
    VPN_LAUNCH_CHECK();
    VPN_LAUNCH(ragged_base_kernel, dim3((unsigned)((S + RS_BLOCK / 64 - 1) / (RS_BLOCK / 64))), dim3(RS_BLOCK), 0, s, chunk_offset, S, C,
               cinc, total);
    VPN_LAUNCH_CHECK();
    VPN_LAUNCH(ragged_sample_kernel, dim3((unsigned)((n + RS_BLOCK - 1) / RS_BLOCK), (unsigned)(S * T)), dim3(RS_BLOCK), 0, s, verts, faces,
               vert_offset, face_offset, chunk_offset, chunks, xforms, xform_mask, u, seed, seed_dev, mesh_base, S, T, n, sumP, sumF, C,
               (const double*)local, (const double*)cinc, (const float*)total, points, face_idx, bary);
    VPN_LAUNCH_CHECK();
    return 0;
}
