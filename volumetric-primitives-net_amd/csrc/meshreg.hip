// meshreg.hip — the three surface priors of a mesh-deformation stage on one face topology shared by the batch (DESIGN.md
// 4.26): edge length, uniform Laplacian (squared), normal consistency.  verts [B,V,3] fp32; every table is int32 and built
// on the host (ops.mesh_topology).
//
//   meshreg_fwd_kernel     one workgroup per (256-item chunk, sample); work-item i of a chunk takes edge i, vertex i and face
//                          i.  Edge: (|v_a - v_b| - l0)^2, as |d|^2 without the root when l0 == 0.  Vertex: delta_i = mean of
//                          the neighbours (CSR order) - v_i, 0 for a vertex in no edge; written for the backward.  Face:
//                          n_f = (v1 - v0) x (v2 - v0), written for the backward; each adjacent face g > f (at most one an
//                          edge, with the sign of the pair) gives 1 - s n_f.n_g / (max(|n_f|, 1e-8) max(|n_g|, 1e-8)), n_g
//                          formed by the same code from g's vertices.  The three sums of the chunk: the butterfly of a wave,
//                          then the four waves in order through LDS.
//   meshreg_final_kernel   one wave: lane l adds chunk sums l, l + 64, ... in order, the butterfly, the scale 1 / count.
//   meshreg_bwd_kernel     a gather, one work-item per (vertex, sample): the neighbours (edge and Laplacian terms, delta and
//                          the degrees read back), then the incident (face, corner) list: the gradient of every pair of the
//                          face with respect to n_f from the saved normals, crossed with the face's edges.  The upstream
//                          gradient [3] is read from the device.
//
// No atomics, no host synchronisation, nothing allocated: the sums have a fixed order, the results are bit-equal from run to
// run.  A term whose bit is absent from `terms` costs nothing, gives 0 and adds nothing to the gradient.
#include "vpn_common.h"

namespace vpn {

constexpr int MESHREG_CHUNK = VPN_MESHREG_CHUNK;   // items per workgroup of the forward
constexpr int MESHREG_BWD_BLOCK = 64;              // vertices per workgroup of the backward: a wave, so B V / 64 workgroups
constexpr float MESHREG_NORM_FLOOR = 1e-8f;

struct V3 { float x, y, z; };
__device__ inline V3 mr_ld(const float* p, long long i) { const F3 f = ld3(p + 3 * i); return V3{f.x, f.y, f.z}; }
__device__ inline V3 mr_sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline float mr_dot(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ inline V3 mr_cross(V3 a, V3 b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// the normal of face f of the sample whose vertices start at v
__device__ inline V3 mr_normal(const float* v, const int* __restrict__ faces, int f) {
    const V3 p0 = mr_ld(v, faces[3 * f]), p1 = mr_ld(v, faces[3 * f + 1]), p2 = mr_ld(v, faces[3 * f + 2]);
    return mr_cross(mr_sub(p1, p0), mr_sub(p2, p0));
}

__global__ __launch_bounds__(256) void meshreg_fwd_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const int* __restrict__ edges, const int* __restrict__ nbr_ptr,
                                                          const int* __restrict__ nbr, const int* __restrict__ adj, int V,
                                                          int E, int F, int chunks, float l0, int terms,
                                                          float* __restrict__ delta, float* __restrict__ normals,
                                                          float* __restrict__ partial) {
    __shared__ float s_part[3][4];
    const int t = threadIdx.x, c = blockIdx.x, b = blockIdx.y, i = c * MESHREG_CHUNK + t;
    const float* v = verts + (long long)b * V * 3;
    float se = 0.0f, sl = 0.0f, sn = 0.0f;
    if ((terms & VPN_MESHREG_EDGE) && i < E) {
        const V3 d = mr_sub(mr_ld(v, edges[2 * i]), mr_ld(v, edges[2 * i + 1]));
        const float q = mr_dot(d, d);
        if (l0 == 0.0f) {
            se = q;
        } else {
            const float r = sqrtf(q) - l0;
            se = r * r;
        }
    }
    if ((terms & VPN_MESHREG_LAP) && i < V) {
        const int e0 = nbr_ptr[i], e1 = nbr_ptr[i + 1];
        V3 d = V3{0.0f, 0.0f, 0.0f};
        if (e1 > e0) {
            V3 s = V3{0.0f, 0.0f, 0.0f};
            for (int e = e0; e < e1; ++e) {
                const V3 p = mr_ld(v, nbr[e]);
                s.x += p.x; s.y += p.y; s.z += p.z;
            }
            const float inv = 1.0f / (float)(e1 - e0);
            const V3 p = mr_ld(v, i);
            d = V3{s.x * inv - p.x, s.y * inv - p.y, s.z * inv - p.z};
        }
        if (delta) st3(delta + ((long long)b * V + i) * 3, d.x, d.y, d.z);
        sl = mr_dot(d, d);
    }
    if ((terms & VPN_MESHREG_NORMAL) && i < F) {
        const V3 nf = mr_normal(v, faces, i);
        if (normals) st3(normals + ((long long)b * F + i) * 3, nf.x, nf.y, nf.z);
        const float lf = fmaxf(sqrtf(mr_dot(nf, nf)), MESHREG_NORM_FLOOR);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int a = adj[3 * i + j];
            if (a < 0 || (a >> 1) <= i) continue;              // no pair across this edge, or the pair is the other face's
            const V3 ng = mr_normal(v, faces, a >> 1);
            const float lg = fmaxf(sqrtf(mr_dot(ng, ng)), MESHREG_NORM_FLOOR);
            const float cs = mr_dot(nf, ng) / (lf * lg);
            sn += 1.0f - ((a & 1) ? -cs : cs);
        }
    }
    se = wave_sum(se); sl = wave_sum(sl); sn = wave_sum(sn);
    if ((t & 63) == 0) { s_part[0][t >> 6] = se; s_part[1][t >> 6] = sl; s_part[2][t >> 6] = sn; }
    __syncthreads();
    if (t < 3) partial[((long long)b * chunks + c) * 3 + t] = ((s_part[t][0] + s_part[t][1]) + s_part[t][2]) + s_part[t][3];
}

// out [3] = the chunk sums added in a fixed order, over the number of (sample, item) each term averages
__global__ __launch_bounds__(64) void meshreg_final_kernel(const float* __restrict__ partial, int n, float inv_e, float inv_l,
                                                           float inv_n, float* __restrict__ out) {
    const int lane = threadIdx.x;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int p = lane; p < n; p += 64) { s0 += partial[3 * (long long)p]; s1 += partial[3 * (long long)p + 1]; s2 += partial[3 * (long long)p + 2]; }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane == 0) { out[0] = s0 * inv_e; out[1] = s1 * inv_l; out[2] = s2 * inv_n; }
}

// we, wl, wn: 2 / (B E), 2 / (B V), 1 / (B pairs), or 0 for a term that is off
__global__ __launch_bounds__(MESHREG_BWD_BLOCK) void meshreg_bwd_kernel(
    const float* __restrict__ gout, const float* __restrict__ verts, const float* __restrict__ delta,
    const float* __restrict__ normals, const int* __restrict__ faces, const int* __restrict__ nbr_ptr,
    const int* __restrict__ nbr, const int* __restrict__ vf_ptr, const int* __restrict__ vf, const int* __restrict__ adj, int V,
    int F, float l0, int terms, float we, float wl, float wn, float* __restrict__ dverts) {
    const int k = blockIdx.x * MESHREG_BWD_BLOCK + threadIdx.x, b = blockIdx.y;
    if (k >= V) return;
    const float* v = verts + (long long)b * V * 3;
    const V3 pk = mr_ld(v, k);
    V3 ge = V3{0.0f, 0.0f, 0.0f}, gl = ge, gn = ge;
    if (terms & (VPN_MESHREG_EDGE | VPN_MESHREG_LAP)) {
        const float* dl = (terms & VPN_MESHREG_LAP) ? delta + (long long)b * V * 3 : nullptr;
        const int e0 = nbr_ptr[k], e1 = nbr_ptr[k + 1];
        for (int e = e0; e < e1; ++e) {
            const int j = nbr[e];
            if (terms & VPN_MESHREG_EDGE) {
                const V3 d = mr_sub(pk, mr_ld(v, j));
                float c = 1.0f;
                if (l0 != 0.0f) {
                    const float len = sqrtf(mr_dot(d, d));
                    c = len > 0.0f ? 1.0f - l0 / len : 0.0f;    // an edge of length 0 has gradient 0
                }
                ge.x = fmaf(c, d.x, ge.x); ge.y = fmaf(c, d.y, ge.y); ge.z = fmaf(c, d.z, ge.z);
            }
            if (terms & VPN_MESHREG_LAP) {
                const float inv = 1.0f / (float)(nbr_ptr[j + 1] - nbr_ptr[j]);      // j has k for a neighbour: its degree is >= 1
                const V3 dj = mr_ld(dl, j);
                gl.x = fmaf(dj.x, inv, gl.x); gl.y = fmaf(dj.y, inv, gl.y); gl.z = fmaf(dj.z, inv, gl.z);
            }
        }
        if ((terms & VPN_MESHREG_LAP) && e1 > e0) {
            const V3 dk = mr_ld(dl, k);
            gl.x -= dk.x; gl.y -= dk.y; gl.z -= dk.z;
        }
    }
    if (terms & VPN_MESHREG_NORMAL) {
        const float* nr = normals + (long long)b * F * 3;
        const int x1 = vf_ptr[k + 1];
        for (int x = vf_ptr[k]; x < x1; ++x) {
            const int f = vf[x] >> 2, corner = vf[x] & 3;
            const V3 nf = mr_ld(nr, f);
            const float rf = sqrtf(mr_dot(nf, nf)), lf = fmaxf(rf, MESHREG_NORM_FLOOR);
            const float own = rf > MESHREG_NORM_FLOOR ? 1.0f / (lf * lf) : 0.0f;      // a clamped norm is a constant
            V3 G = V3{0.0f, 0.0f, 0.0f};                                           // d sum(1 - cos) / d n_f
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int a = adj[3 * f + j];
                if (a < 0) continue;
                const V3 ng = mr_ld(nr, a >> 1);
                const float lg = fmaxf(sqrtf(mr_dot(ng, ng)), MESHREG_NORM_FLOOR);
                const float inv = ((a & 1) ? -1.0f : 1.0f) / (lf * lg), q = mr_dot(nf, ng) * own;
                G.x -= inv * (ng.x - q * nf.x); G.y -= inv * (ng.y - q * nf.y); G.z -= inv * (ng.z - q * nf.z);
            }
            const V3 p0 = mr_ld(v, faces[3 * f]), p1 = mr_ld(v, faces[3 * f + 1]), p2 = mr_ld(v, faces[3 * f + 2]);
            const V3 g1 = mr_cross(mr_sub(p2, p0), G), g2 = mr_cross(G, mr_sub(p1, p0));   // d / d v1, d / d v2
            if (corner == 1) { gn.x += g1.x; gn.y += g1.y; gn.z += g1.z; }
            else if (corner == 2) { gn.x += g2.x; gn.y += g2.y; gn.z += g2.z; }
            else { gn.x -= g1.x + g2.x; gn.y -= g1.y + g2.y; gn.z -= g1.z + g2.z; }
        }
    }
    const float ce = gout[0] * we, cl = gout[1] * wl, cn = gout[2] * wn;
    float rx = 0.0f, ry = 0.0f, rz = 0.0f;                     // a term that is off adds nothing, whatever its upstream gradient
    if (terms & VPN_MESHREG_EDGE) { rx = ce * ge.x; ry = ce * ge.y; rz = ce * ge.z; }
    if (terms & VPN_MESHREG_LAP) { rx = fmaf(cl, gl.x, rx); ry = fmaf(cl, gl.y, ry); rz = fmaf(cl, gl.z, rz); }
    if (terms & VPN_MESHREG_NORMAL) { rx = fmaf(cn, gn.x, rx); ry = fmaf(cn, gn.y, ry); rz = fmaf(cn, gn.z, rz); }
    st3(dverts + ((long long)b * V + k) * 3, rx, ry, rz);
}

}  // namespace vpn

using namespace vpn;

// the shapes both entries take: 0, or the code of the first rule they break
static int meshreg_check(int B, int V, int E, int F, int P, float l0, int terms) {
    if (B <= 0 || V <= 0 || F <= 0 || E < 0 || P < 0 || terms < 0 || terms > 7 || !(l0 >= 0.0f) || !(l0 <= 3.0e38f))
        return VPN_E_BADARG;
    if (B > 65535 || V > VPN_MESHREG_MAX_ITEMS || E > VPN_MESHREG_MAX_ITEMS || F > VPN_MESHREG_MAX_ITEMS) return VPN_E_TOOBIG;
    return 0;
}

static int meshreg_chunks(int V, int E, int F) {
    const int m = V > E ? (V > F ? V : F) : (E > F ? E : F);
    return (m + MESHREG_CHUNK - 1) / MESHREG_CHUNK;
}

// a term with nothing to average is off: its value is 0 and its gradient nothing
static int meshreg_live_terms(int terms, int E, int P) {
    if (E == 0) terms &= ~(VPN_MESHREG_EDGE | VPN_MESHREG_LAP);
    if (P == 0) terms &= ~VPN_MESHREG_NORMAL;
    return terms;
}

extern "C" size_t vpn_meshreg_workspace(int B, int V, int E, int F) {
    if (meshreg_check(B, V, E, F, 0, 0.0f, 0)) return 0;
    return (size_t)B * meshreg_chunks(V, E, F) * 3 * sizeof(float);
}

extern "C" int vpn_meshreg_fwd(const float* verts, const int32_t* faces, const int32_t* edges, const int32_t* nbr_ptr,
                               const int32_t* nbr, const int32_t* adj, int B, int V, int E, int F, int P, float edge_target,
                               int terms, void* workspace, float* delta, float* normals, float* out, void* stream) {
    if (!verts || !faces || !nbr_ptr || !adj || !workspace || !out || (E > 0 && (!edges || !nbr))) return VPN_E_BADARG;
    const int rc = meshreg_check(B, V, E, F, P, edge_target, terms);
    if (rc) return rc;
    terms = meshreg_live_terms(terms, E, P);
    const int chunks = meshreg_chunks(V, E, F);
    float* part = (float*)workspace;
    VPN_LAUNCH(meshreg_fwd_kernel, dim3(chunks, B), dim3(256), 0, (hipStream_t)stream, verts, (const int*)faces,
               (const int*)edges, (const int*)nbr_ptr, (const int*)nbr, (const int*)adj, V, E, F, chunks, edge_target, terms,
               delta, normals, part);
    const float inv_e = (terms & VPN_MESHREG_EDGE) ? (float)(1.0 / ((double)B * E)) : 0.0f;
    const float inv_l = (terms & VPN_MESHREG_LAP) ? (float)(1.0 / ((double)B * V)) : 0.0f;
    const float inv_n = (terms & VPN_MESHREG_NORMAL) ? (float)(1.0 / ((double)B * P)) : 0.0f;
    VPN_LAUNCH(meshreg_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)part, B * chunks, inv_e, inv_l,
               inv_n, out);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" int vpn_meshreg_bwd(const float* grad, const float* verts, const float* delta, const float* normals,
                               const int32_t* faces, const int32_t* nbr_ptr, const int32_t* nbr, const int32_t* vf_ptr,
                               const int32_t* vf, const int32_t* adj, int B, int V, int E, int F, int P, float edge_target,
                               int terms, float* dverts, void* stream) {
    if (!grad || !verts || !faces || !nbr_ptr || !vf_ptr || !adj || !dverts || (E > 0 && !nbr)) return VPN_E_BADARG;
    const int rc = meshreg_check(B, V, E, F, P, edge_target, terms);
    if (rc) return rc;
    terms = meshreg_live_terms(terms, E, P);
    if (((terms & VPN_MESHREG_LAP) && !delta) || ((terms & VPN_MESHREG_NORMAL) && (!normals || !vf))) return VPN_E_BADARG;
    const float we = (terms & VPN_MESHREG_EDGE) ? (float)(2.0 / ((double)B * E)) : 0.0f;
    const float wl = (terms & VPN_MESHREG_LAP) ? (float)(2.0 / ((double)B * V)) : 0.0f;
    const float wn = (terms & VPN_MESHREG_NORMAL) ? (float)(1.0 / ((double)B * P)) : 0.0f;
    VPN_LAUNCH(meshreg_bwd_kernel, dim3((V + MESHREG_BWD_BLOCK - 1) / MESHREG_BWD_BLOCK, B), dim3(MESHREG_BWD_BLOCK), 0,
               (hipStream_t)stream, grad, verts, delta, normals, (const int*)faces, (const int*)nbr_ptr, (const int*)nbr,
               (const int*)vf_ptr, (const int*)vf, (const int*)adj, V, F, edge_target, terms, we, wl, wn, dverts);
    VPN_LAUNCH_CHECK();
    return 0;
}
