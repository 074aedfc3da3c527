// isosurface.hip — outer-surface extraction: the implicit field of a primitive assembly and surface nets on a
// lattice, an operator whose output size depends on the data.
//
//   prim_field_kernel   one work-item per (query, sample): f = min_k (m_k - 1) with m_k as occ_prims_kernel forms it (the pose
//                       records and x~ come from occupancy_prim.h), a NaN m_k skipped, +inf when nothing is left.
//   iso_count_kernel    one work-item per lattice cell in workgroups of 256: the inside mask of the 8 corners, whether the cell
//                       is active, the quads it owns and the open edges it answers for; ballots and popcounts per wave, the four
//                       waves through LDS, one row of sums per workgroup.
//   iso_scan_kernel     one workgroup per sample: the exclusive scan of the rows (a work-item owns a run of ceil(rows / 256)
//                       consecutive rows, the 256 run totals are scanned in LDS), in place; the counts and the overflow flag.
//   iso_vertex_kernel   the grid of the count: the rank of an active cell = its row's offset + its rank in the workgroup (ballots
//                       again); the vertex of the cell and the cell -> vertex table; the padding rows.
//   iso_face_kernel     the same grid: the quads a cell owns, from the table; the padding rows.
//
// No atomics, no scratch, no hand-off between workgroups of a launch, nothing allocated: counts are integers, every rank
// follows from the cell index, every vertex is one fixed chain of fp32 operations, so the results are bit-equal from run to run.
//
// Workspace (vpn_isosurface_workspace): rows int32 [B][blocks][4] = (active cells, quads, open edges, 0), after the scan
// (vertices before the row, quads before the row, -, -); then the table int32 [B][cells], written for active cells only (no
// other entry is ever read: a sign-changing edge makes the four cells around it active).
//
// Built with -ffp-contract=off: every product, sum and quotient is rounded by itself, as tests/isosurface_ref.py states them.
#include "vpn_common.h"
#include "occupancy_prim.h"
#include <float.h>

namespace {

constexpr int IS_TILE = VPN_OCCUPANCY_TILE;             // queries, and cells, per workgroup
constexpr int IS_MAX_ITEMS = VPN_OCCUPANCY_MAX_ITEMS;
using vpn::OC_STAGE;
using vpn::OcPrim;

// queries [Q,3] (q_stride 0) or [B,Q,3] (q_stride 3 Q); f [B,Q]
__global__ __launch_bounds__(256) void prim_field_kernel(const float* __restrict__ params, const int32_t* __restrict__ kinds,
                                                         const float* __restrict__ queries, long long q_stride, int K, int Q,
                                                         float* __restrict__ f) {
    __shared__ OcPrim s_p[OC_STAGE];
    const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.x * IS_TILE + tid;
    const bool valid = i < Q;
    const vpn::F3 x = valid ? vpn::ld3(queries + (size_t)b * q_stride + (size_t)i * 3) : vpn::F3{0.0f, 0.0f, 0.0f};
    float best = INFINITY;
    for (int base = 0; base < K; base += OC_STAGE) {
        const int m = min(OC_STAGE, K - base);
        __syncthreads();                                 // the previous records have been read
        if (tid < m) vpn::oc_stage_prim(s_p[tid], params, kinds, b, K, base + tid);
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const OcPrim& p = s_p[k];                    // the same address for every lane: an LDS broadcast
            const vpn::F3 y = vpn::oc_local(p, x);
            // the cuboid's max |x~_i| is a NaN where any x~_i is one (fmaxf would drop it): the primitive is skipped, as the
            // occupancy's three comparisons fail
            const float mk = p.sphere ? y.x * y.x + y.y * y.y + y.z * y.z
                                      : ((y.x != y.x || y.y != y.y || y.z != y.z) ? NAN : fmaxf(fabsf(y.x), fmaxf(fabsf(y.y), fabsf(y.z))));
            const float d = mk - 1.0f;                   // <= 0 exactly where m <= 1: a difference of two floats is 0 only when they are equal
            if (d < best) best = d;                      // a NaN fails the comparison
        }
    }
    if (valid) f[(size_t)b * Q + i] = best;
}

// ---- surface nets

struct IsoDims { int Nx, Ny, Nz, ncx, ncy, ncz, cells, blocks; };

inline IsoDims iso_dims(int Nx, int Ny, int Nz) {
    IsoDims d;
    d.Nx = Nx; d.Ny = Ny; d.Nz = Nz; d.ncx = Nx - 1; d.ncy = Ny - 1; d.ncz = Nz - 1;
    d.cells = d.ncx * d.ncy * d.ncz;
    d.blocks = (d.cells + IS_TILE - 1) / IS_TILE;
    return d;
}

// s = field - level, NaN -> +FLT_MAX, clamped to +-FLT_MAX
__device__ inline float iso_value(const float* __restrict__ field, size_t node, float level) {
    float s = field[node] - level;
    if (s != s) s = FLT_MAX;
    return fminf(fmaxf(s, -FLT_MAX), FLT_MAX);
}

struct IsoCell { int c[3]; };
__device__ inline IsoCell iso_cell(const IsoDims& d, int cell) {
    IsoCell k;
    const int t = cell / d.ncx;
    k.c[0] = cell - t * d.ncx; k.c[2] = t / d.ncy; k.c[1] = t - k.c[2] * d.ncy;
    return k;
}
__device__ inline size_t iso_node(const IsoDims& d, const IsoCell& k) { return ((size_t)k.c[2] * d.Ny + k.c[1]) * d.Nx + k.c[0]; }

// corner i = ox + 2 oy + 4 oz of the cell; s[i] its value, bit i of the mask = inside (s <= 0)
__device__ inline unsigned iso_corners(const float* __restrict__ field, float level, const IsoDims& d, const IsoCell& k, float s[8]) {
    const size_t n0 = iso_node(d, k);
    unsigned mask = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s[i] = iso_value(field, n0 + ((size_t)(i >> 2) * d.Ny + ((i >> 1) & 1)) * d.Nx + (i & 1), level);
        mask |= (unsigned)(s[i] <= 0.0f) << i;
    }
    return mask;
}

__device__ inline unsigned iso_changes(unsigned mask, int i, int j) { return ((mask >> i) ^ (mask >> j)) & 1u; }

// bit a: the cell owns the quad of its edge from corner 0 along axis a (the edge changes sign and four cells surround it: the
// cell is not the first along either other axis).  Needs bits 0, 1, 2 and 4 of the mask only.
__device__ inline unsigned iso_owned(unsigned mask, const IsoCell& k) {
    unsigned own = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int u = (a + 1) % 3, v = (a + 2) % 3;
        own |= (iso_changes(mask, 0, 1 << a) & (unsigned)(k.c[u] >= 1) & (unsigned)(k.c[v] >= 1)) << a;
    }
    return own;
}

// the sign-changing edges in a boundary face of the lattice this cell answers for: a lattice edge belongs to the cell at its
// first node, clamped to the last cell along the two other axes (so the far faces are counted once)
__device__ inline int iso_open(unsigned mask, const IsoDims& d, const IsoCell& k) {
    const int nc[3] = {d.ncx, d.ncy, d.ncz};
    int open = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ou = e & 1, ov = e >> 1, i = (ou << u) | (ov << v);
            const bool mine = (ou == 0 || k.c[u] == nc[u] - 1) && (ov == 0 || k.c[v] == nc[v] - 1);
            const bool edge_u = ou ? k.c[u] == nc[u] - 1 : k.c[u] == 0, edge_v = ov ? k.c[v] == nc[v] - 1 : k.c[v] == 0;
            open += (int)(iso_changes(mask, i, i | (1 << a)) & (unsigned)(mine && (edge_u || edge_v)));
        }
    }
    return open;
}

// rows [B][blocks][4] = (active, quads, open, 0) of every workgroup
__global__ __launch_bounds__(256) void iso_count_kernel(const float* __restrict__ field, float level, IsoDims d,
                                                        int32_t* __restrict__ rows) {
    __shared__ int s_w[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, cell = blockIdx.x * IS_TILE + tid;
    unsigned active = 0, own = 0;
    int open = 0;
    if (cell < d.cells) {
        const IsoCell k = iso_cell(d, cell);
        float s[8];
        const unsigned mask = iso_corners(field + (size_t)b * d.Nx * d.Ny * d.Nz, level, d, k, s);
        active = mask != 0u && mask != 255u;
        own = iso_owned(mask, k);
        open = iso_open(mask, d, k);
    }
    const int n_active = __popcll(__ballot(active));
    const int n_quads = __popcll(__ballot(own & 1u)) + __popcll(__ballot(own & 2u)) + __popcll(__ballot(own & 4u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o, 64);
    if (lane == 0) { s_w[wave][0] = n_active; s_w[wave][1] = n_quads; s_w[wave][2] = open; }
    __syncthreads();
    if (tid < 4) rows[((size_t)b * d.blocks + blockIdx.x) * 4 + tid] = tid < 3 ? (s_w[0][tid] + s_w[1][tid]) + (s_w[2][tid] + s_w[3][tid]) : 0;
}

// ONE workgroup per sample.  Work-item t owns rows t per .. t per + per - 1; inclusive scan of the 256 run totals in LDS
// (Hillis and Steele, two buffers); the rows become exclusive offsets in place.  counts [B][4] = (n_verts, n_faces, n_open,
// overflow).
__global__ __launch_bounds__(256) void iso_scan_kernel(int32_t* __restrict__ rows_all, int blocks, int max_verts, int max_faces,
                                                       int32_t* __restrict__ counts) {
    __shared__ unsigned long long s_vq[2][256];          // vertices in the low word, quads in the high one: neither reaches 2^32
    __shared__ int s_open[2][256];
    const int tid = threadIdx.x, b = blockIdx.x;
    int32_t* rows = rows_all + (size_t)b * blocks * 4;
    const int per = (blocks + 255) / 256, j0 = min(tid * per, blocks), j1 = min(j0 + per, blocks);
    unsigned long long vq = 0;
    int open = 0;
    for (int j = j0; j < j1; ++j) {
        vq += (unsigned long long)(unsigned)rows[(size_t)j * 4] | ((unsigned long long)(unsigned)rows[(size_t)j * 4 + 1] << 32);
        open += rows[(size_t)j * 4 + 2];
    }
    int cur = 0;
    s_vq[0][tid] = vq; s_open[0][tid] = open;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < 256; o <<= 1) {
        unsigned long long a = s_vq[cur][tid];
        int c = s_open[cur][tid];
        if (tid >= o) { a += s_vq[cur][tid - o]; c += s_open[cur][tid - o]; }
        s_vq[cur ^ 1][tid] = a; s_open[cur ^ 1][tid] = c;
        cur ^= 1;
        __syncthreads();
    }
    unsigned long long run = s_vq[cur][tid] - vq;        // before this work-item's rows
    for (int j = j0; j < j1; ++j) {
        const unsigned long long mine = (unsigned long long)(unsigned)rows[(size_t)j * 4] | ((unsigned long long)(unsigned)rows[(size_t)j * 4 + 1] << 32);
        rows[(size_t)j * 4] = (int32_t)(unsigned)(run & 0xffffffffull);
        rows[(size_t)j * 4 + 1] = (int32_t)(unsigned)(run >> 32);
        run += mine;
    }
    if (tid == 255) {
        const unsigned long long total = s_vq[cur][255];
        const long long n_verts = (long long)(total & 0xffffffffull), n_faces = 2 * (long long)(total >> 32);
        counts[(size_t)b * 4 + 0] = (int32_t)n_verts;
        counts[(size_t)b * 4 + 1] = (int32_t)n_faces;
        counts[(size_t)b * 4 + 2] = s_open[cur][255];
        counts[(size_t)b * 4 + 3] = n_verts > max_verts || n_faces > max_faces;
    }
}

// verts [B][max_verts][3]; table [B][cells]
__global__ __launch_bounds__(256) void iso_vertex_kernel(const float* __restrict__ field, const float* __restrict__ cx,
                                                         const float* __restrict__ cy, const float* __restrict__ cz, float level,
                                                         IsoDims d, const int32_t* __restrict__ rows, const int32_t* __restrict__ counts,
                                                         int max_verts, float* __restrict__ verts, int32_t* __restrict__ table) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, cell = blockIdx.x * IS_TILE + tid;
    const bool overflow = counts[(size_t)b * 4 + 3] != 0;
    const int n_verts = overflow ? 0 : counts[(size_t)b * 4];
    float s[8];
    unsigned mask = 0;
    IsoCell k = IsoCell{{0, 0, 0}};
    if (cell < d.cells) {
        k = iso_cell(d, cell);
        mask = iso_corners(field + (size_t)b * d.Nx * d.Ny * d.Nz, level, d, k, s);
    }
    const bool active = mask != 0u && mask != 255u;
    const unsigned long long vote = __ballot(active);
    if (lane == 0) s_w[wave] = __popcll(vote);
    __syncthreads();
    if (active && !overflow) {
        int rank = rows[((size_t)b * d.blocks + blockIdx.x) * 4] + __popcll(vote & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += s_w[w];
        const float lo[3] = {cx[k.c[0]], cy[k.c[1]], cz[k.c[2]]}, hi[3] = {cx[k.c[0] + 1], cy[k.c[1] + 1], cz[k.c[2] + 1]};
        float sum[3] = {0.0f, 0.0f, 0.0f};
        int n = 0;
        // the edges in ONE order: axis x, y, z; within an axis the offsets (0,0), (1,0), (0,1), (1,1) along the two other
        // axes taken cyclically (x: y z, y: z x, z: x y)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ou = e & 1, ov = e >> 1, i = (ou << u) | (ov << v), j = i | (1 << a);
                if (iso_changes(mask, i, j)) {
                    const float t = s[i] / (s[i] - s[j]);                      // in [0,1]: the two values differ in sign
                    float p[3];
                    p[a] = lo[a] + t * (hi[a] - lo[a]);
                    p[u] = ou ? hi[u] : lo[u];
                    p[v] = ov ? hi[v] : lo[v];
                    sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2];
                    ++n;
                }
            }
        }
        const float fn = (float)n;
        vpn::st3(verts + ((size_t)b * max_verts + rank) * 3, sum[0] / fn, sum[1] / fn, sum[2] / fn);
        table[(size_t)b * d.cells + cell] = rank;
    }
    const long long stride = (long long)d.blocks * IS_TILE;
    for (long long r = n_verts + (long long)blockIdx.x * IS_TILE + tid; r < max_verts; r += stride)
        vpn::st3(verts + ((size_t)b * max_verts + r) * 3, 0.0f, 0.0f, 0.0f);
}

// faces [B][max_faces][3], mesh-local
__global__ __launch_bounds__(256) void iso_face_kernel(const float* __restrict__ field, float level, IsoDims d,
                                                       const int32_t* __restrict__ rows, const int32_t* __restrict__ counts,
                                                       const int32_t* __restrict__ table, int max_faces, int32_t* __restrict__ faces) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, cell = blockIdx.x * IS_TILE + tid;
    const bool overflow = counts[(size_t)b * 4 + 3] != 0;
    const int n_faces = overflow ? 0 : counts[(size_t)b * 4 + 1];
    unsigned mask = 0, own = 0;
    IsoCell k = IsoCell{{0, 0, 0}};
    if (cell < d.cells) {
        k = iso_cell(d, cell);
        const float* f = field + (size_t)b * d.Nx * d.Ny * d.Nz;
        const size_t n0 = iso_node(d, k);
        mask = (unsigned)(iso_value(f, n0, level) <= 0.0f) | (unsigned)(iso_value(f, n0 + 1, level) <= 0.0f) << 1 |
               (unsigned)(iso_value(f, n0 + d.Nx, level) <= 0.0f) << 2 | (unsigned)(iso_value(f, n0 + (size_t)d.Nx * d.Ny, level) <= 0.0f) << 4;
        own = iso_owned(mask, k);
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long vx = __ballot(own & 1u), vy = __ballot(own & 2u), vz = __ballot(own & 4u);
    if (lane == 0) s_w[wave] = __popcll(vx) + __popcll(vy) + __popcll(vz);
    __syncthreads();
    if (own && !overflow) {
        int quad = rows[((size_t)b * d.blocks + blockIdx.x) * 4 + 1] + __popcll(vx & below) + __popcll(vy & below) + __popcll(vz & below);
        for (int w = 0; w < wave; ++w) quad += s_w[w];
        const int32_t* tb = table + (size_t)b * d.cells;
        const int step[3] = {1, d.ncx, d.ncx * d.ncy};    // the cell index along x, y, z
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(own & (1u << a))) continue;
            // the four cells around the edge, counter-clockwise seen from its positive direction: offsets (-,-), (0,-), (0,0),
            // (-,0) in the cyclic plane (u, v)
            const int u = (a + 1) % 3, v = (a + 2) % 3;
            const int c0 = tb[cell - step[u] - step[v]], c1 = tb[cell - step[v]], c2 = tb[cell], c3 = tb[cell - step[u]];
            const bool out = mask & 1u;                   // the edge runs from inside to outside: the normal is its direction
            int32_t* fc = faces + ((size_t)b * max_faces + 2 * (size_t)quad) * 3;
            fc[0] = c0; fc[1] = out ? c1 : c3; fc[2] = c2;
            fc[3] = c0; fc[4] = c2; fc[5] = out ? c3 : c1;
            ++quad;
        }
    }
    const long long stride = (long long)d.blocks * IS_TILE;
    for (long long r = n_faces + (long long)blockIdx.x * IS_TILE + tid; r < max_faces; r += stride) {
        int32_t* fc = faces + ((size_t)b * max_faces + r) * 3;
        fc[0] = 0; fc[1] = 0; fc[2] = 0;
    }
}

struct IsoLayout { size_t rows, table, total; };
inline IsoLayout iso_layout(int B, const IsoDims& d) {
    IsoLayout L;
    L.rows = 0;
    L.table = (size_t)B * d.blocks * 4 * sizeof(int32_t);                      // a multiple of 16
    L.total = (L.table + (size_t)B * d.cells * sizeof(int32_t) + 15) & ~(size_t)15;
    return L;
}

int iso_check(int B, int Nx, int Ny, int Nz) {
    if (B <= 0 || Nx < 2 || Ny < 2 || Nz < 2) return VPN_E_BADARG;
    if (B > 65535 || (long long)Nx * Ny > IS_MAX_ITEMS || (long long)Nx * Ny * Nz > IS_MAX_ITEMS) return VPN_E_TOOBIG;
    return 0;
}

}  // namespace

extern "C" int vpn_primitive_field(const float* params, const int32_t* kinds, const float* queries, int shared_queries, int B, int K,
                                   int Q, float* f, void* stream) {
    if (!params || !kinds || !queries || !f) return VPN_E_BADARG;
    if (B <= 0 || K <= 0 || Q <= 0) return VPN_E_BADARG;
    if (B > 65535 || Q > IS_MAX_ITEMS || K > VPN_MAX_PRIMS) return VPN_E_TOOBIG;
    VPN_LAUNCH(prim_field_kernel, dim3((Q + IS_TILE - 1) / IS_TILE, B), dim3(256), 0, (hipStream_t)stream, params, kinds, queries,
               shared_queries ? 0LL : 3LL * Q, K, Q, f);
    VPN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vpn_isosurface_workspace(int B, int Nx, int Ny, int Nz) {
    if (iso_check(B, Nx, Ny, Nz)) return 0;
    return iso_layout(B, iso_dims(Nx, Ny, Nz)).total;
}

extern "C" int vpn_isosurface(const float* field, const float* cx, const float* cy, const float* cz, float level, int B, int Nx,
                              int Ny, int Nz, int max_verts, int max_faces, void* workspace, size_t workspace_bytes, float* verts,
                              int32_t* faces, int32_t* counts, void* stream) {
    if (!field || !cx || !cy || !cz || !workspace || !verts || !faces || !counts) return VPN_E_BADARG;
    if (!(fabsf(level) <= FLT_MAX) || max_verts <= 0 || max_faces <= 0) return VPN_E_BADARG;
    const int rc = iso_check(B, Nx, Ny, Nz);
    if (rc) return rc;
    if (max_verts > IS_MAX_ITEMS || max_faces > IS_MAX_ITEMS) return VPN_E_TOOBIG;
    const IsoDims d = iso_dims(Nx, Ny, Nz);
    const IsoLayout L = iso_layout(B, d);
    if (workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(workspace) & 15)) return VPN_E_BADARG;
    int32_t* rows = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.rows);
    int32_t* table = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.table);
    hipStream_t s = (hipStream_t)stream;
    VPN_LAUNCH(iso_count_kernel, dim3(d.blocks, B), dim3(256), 0, s, field, level, d, rows);
    VPN_LAUNCH(iso_scan_kernel, dim3(B), dim3(256), 0, s, rows, d.blocks, max_verts, max_faces, counts);
    VPN_LAUNCH(iso_vertex_kernel, dim3(d.blocks, B), dim3(256), 0, s, field, cx, cy, cz, level, d, (const int32_t*)rows,
               (const int32_t*)counts, max_verts, verts, table);
    VPN_LAUNCH(iso_face_kernel, dim3(d.blocks, B), dim3(256), 0, s, field, level, d, (const int32_t*)rows, (const int32_t*)counts,
               (const int32_t*)table, max_faces, faces);
    VPN_LAUNCH_CHECK();
    return 0;
}
