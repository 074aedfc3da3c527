// Host check of the outer-surface extraction (csrc/isosurface.hip) without a GPU, in the manner of
// tools/occupancy_host: the five kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers) and compared with a double statement of the
// definitions: the field against min_k (m_k - 1), the extraction against plain loops over cells and edges (counts, open
// edges, faces and padding exact, vertices within 1e-6).  Inputs include lattice
// dimensions that are no multiple of the workgroup, more workgroups than the scan has work-items, NaN and inf nodes, a level
// that is not 0, capacities equal to and one below the counts, an empty and an all-inside sample, more primitives than one
// staging; and every rejected argument.  Every buffer has its exact size, so AddressSanitizer sees any access past an end.  It
// checks indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/isosurface_host/main.cpp -o isosurface_host
//   ./isosurface_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
// the wave operations the shim lacks: an int travels through a buffer of its own; a ballot is the OR of every lane's bit
static int g_xi[16][64];
inline int __shfl_xor(int v, int o, int) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xi[w][l] = v; g_wave[w].wait(); const int r = g_xi[w][l ^ o]; g_wave[w].wait(); return r;
}
inline unsigned long long __ballot(int pred) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xi[w][l] = pred != 0; g_wave[w].wait();
    unsigned long long r = 0;
    for (int k = 0; k < 64; ++k) r |= (unsigned long long)(g_xi[w][k] != 0) << k;
    g_wave[w].wait(); return r;
}
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
#include "../../volumetric-primitives-net_amd/csrc/isosurface.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <chrono>
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(31);
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
template <class T> static T* alv(const std::vector<T>& v) { T* p = al<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }
static void* al16(size_t bytes) { void* p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 16)) return nullptr; return p; }   // exact size, 16-byte aligned

// ---- the field: the definition in double on the fp32 inputs
static void rotation64(const float* q, double R[3][3]) {
    const double PI32 = 3.1415927410125732;
    const double r = (double)q[3] - floor((double)q[3]), h = ((r * 2) * PI32) / 2;
    const double a = q[0] * sin(h), b = q[1] * sin(h), c = q[2] * sin(h), d = cos(h), l = sqrt(a * a + b * b + c * c + d * d);
    const double x = a / l, y = b / l, z = c / l, w = d / l;
    R[0][0] = x * x - y * y - z * z + w * w; R[0][1] = 2 * (x * y - z * w); R[0][2] = 2 * (x * z + y * w);
    R[1][0] = 2 * (x * y + z * w); R[1][1] = -x * x + y * y - z * z + w * w; R[1][2] = 2 * (y * z - x * w);
    R[2][0] = 2 * (x * z - y * w); R[2][1] = 2 * (y * z + x * w); R[2][2] = -x * x - y * y + z * z + w * w;
}
static double prim_m64(const float* prm, bool sphere, const float* x) {
    double R[3][3]; rotation64(prm + 3, R);
    const double d[3] = {(double)x[0] - prm[7], (double)x[1] - prm[8], (double)x[2] - prm[9]};
    double y[3];
    for (int i = 0; i < 3; ++i) y[i] = (R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2]) / prm[i];
    if (std::isnan(y[0]) || std::isnan(y[1]) || std::isnan(y[2])) return NAN;
    return sphere ? y[0] * y[0] + y[1] * y[1] + y[2] * y[2] : std::max(fabs(y[0]), std::max(fabs(y[1]), fabs(y[2])));
}

static int run_field(const char* name, int B, int K, int Q, bool shared, bool hostile) {
    std::uniform_real_distribution<float> ud(-0.5f, 0.5f), uv(0.1f, 0.4f);
    std::vector<float> params((size_t)B * K * 10), q((size_t)(shared ? 1 : B) * Q * 3);
    std::vector<int> kinds(K);
    for (int i = 0; i < B * K; ++i) { float* p = &params[(size_t)i * 10]; for (int k = 0; k < 3; ++k) p[k] = uv(rng); for (int k = 3; k < 7; ++k) p[k] = 2 * ud(rng); for (int k = 7; k < 10; ++k) p[k] = 0.6f * ud(rng); }
    for (int& k : kinds) k = rng() % 2;
    for (float& x : q) x = 1.2f * ud(rng);
    if (hostile) {      // a NaN and an inf query, a zero extent, a NaN extent, an inf quaternion; ALL primitives of the last sample NaN
        q[0] = NAN; q[4] = INFINITY; params[0] = 0.0f; params[10 + 1] = NAN; params[(size_t)K * 10 + 3] = INFINITY;
        for (int k = 0; k < K; ++k) params[((size_t)(B - 1) * K + k) * 10 + 7] = NAN;
    }
    float *d_p = alv(params), *d_q = alv(q); int* d_k = alv(kinds);
    float* f = al<float>((size_t)B * Q);
    bool ok = vpn_primitive_field(d_p, d_k, d_q, shared, B, K, Q, f, nullptr) == 0;
    double worst = 0; int skipped = 0, infinite = 0, inside = 0, wrong = 0;
    for (int b = 0; b < B && ok; ++b) for (int i = 0; i < Q; ++i) {
        const float* x = &q[((size_t)(shared ? 0 : b) * Q + i) * 3];
        double want = INFINITY; bool near_nan = false;
        for (int k = 0; k < K; ++k) {
            const double m = prim_m64(&params[((size_t)b * K + k) * 10], kinds[k] == VPN_SPHERE, x);
            if (std::isnan(m)) { ++skipped; continue; }
            if (!std::isfinite(m)) near_nan = true;          // inf in double may be inf - inf = NaN in fp32 (and the other way): not compared
            want = std::min(want, m - 1);
        }
        const float got = f[(size_t)b * Q + i];
        if (std::isnan(got)) { ++wrong; continue; }                                   // the field is never a NaN
        inside += got <= 0;
        if (near_nan) continue;
        if (std::isinf(want)) { ++infinite; wrong += !(std::isinf(got) && got > 0); continue; }
        if (std::isinf(got)) { ++wrong; continue; }
        worst = std::max(worst, fabs(got - want) / (1 + fabs(want)));
    }
    ok = ok && wrong == 0 && worst <= 1e-4;
    printf("%-34s B %2d K %3d Q %4d  inside %5d  +inf %4d  skipped (query, primitive) pairs %5d  worst %.2e  wrong %d  %s\n", name, B, K, Q, inside, infinite, skipped, worst, wrong, ok ? "ok" : "FAILED");
    free(d_p); free(d_q); free(d_k); free(f);
    return !ok;
}

// ---- surface nets: plain loops in double on the fp32 inputs
struct Mesh64 { std::vector<double> verts; std::vector<int> faces; int n_open = 0; };
static Mesh64 nets64(const float* field, const std::vector<float> c[3], float level, int Nx, int Ny, int Nz) {
    const int N[3] = {Nx, Ny, Nz};
    auto s = [&](int ix, int iy, int iz) { float v = field[((size_t)iz * Ny + iy) * Nx + ix] - level; if (std::isnan(v)) v = FLT_MAX; return (double)std::min(std::max(v, -FLT_MAX), FLT_MAX); };
    auto sn = [&](const int* n) { return s(n[0], n[1], n[2]); };
    Mesh64 out;
    std::vector<int> number((size_t)(Nx - 1) * (Ny - 1) * (Nz - 1), -1);
    auto cell_index = [&](const int* k) { return ((size_t)k[2] * (Ny - 1) + k[1]) * (Nx - 1) + k[0]; };
    int nv = 0;
    for (int z = 0; z < Nz - 1; ++z) for (int y = 0; y < Ny - 1; ++y) for (int x = 0; x < Nx - 1; ++x) {
        const int k[3] = {x, y, z};
        int inside = 0;
        for (int i = 0; i < 8; ++i) inside += s(x + (i & 1), y + ((i >> 1) & 1), z + (i >> 2)) <= 0;
        if (inside == 0 || inside == 8) continue;
        double sum[3] = {0, 0, 0}; int n = 0;
        for (int a = 0; a < 3; ++a) for (int e = 0; e < 4; ++e) {
            const int u = (a + 1) % 3, v = (a + 2) % 3;
            int na[3] = {k[0], k[1], k[2]}; na[u] += e & 1; na[v] += e >> 1;
            int nb[3] = {na[0], na[1], na[2]}; nb[a] += 1;
            const double sa = sn(na), sb = sn(nb);
            if ((sa <= 0) == (sb <= 0)) continue;
            // fp32 forms s_a - s_b as +-inf when both are clamped extremes: t = 0 there, as the header's definition is read in fp32
            const double den = sa - sb, t = fabs(den) > FLT_MAX ? 0.0 : sa / den;
            double p[3] = {c[0][na[0]], c[1][na[1]], c[2][na[2]]};
            p[a] = (double)c[a][na[a]] + t * ((double)c[a][nb[a]] - (double)c[a][na[a]]);
            for (int r = 0; r < 3; ++r) sum[r] += p[r];
            ++n;
        }
        for (int r = 0; r < 3; ++r) out.verts.push_back(sum[r] / n);
        number[cell_index(k)] = nv++;
    }
    for (int z = 0; z < Nz - 1; ++z) for (int y = 0; y < Ny - 1; ++y) for (int x = 0; x < Nx - 1; ++x) for (int a = 0; a < 3; ++a) {
        const int k[3] = {x, y, z}, u = (a + 1) % 3, v = (a + 2) % 3;
        int nb[3] = {x, y, z}; nb[a] += 1;
        const double sa = sn(k), sb = sn(nb);
        if ((sa <= 0) == (sb <= 0) || k[u] < 1 || k[v] < 1) continue;
        int k0[3] = {x, y, z}, k1[3] = {x, y, z}, k3[3] = {x, y, z};
        k0[u] -= 1; k0[v] -= 1; k1[v] -= 1; k3[u] -= 1;
        const int c0 = number[cell_index(k0)], c1 = number[cell_index(k1)], c2 = number[cell_index(k)], c3 = number[cell_index(k3)];
        if (sa <= 0) out.faces.insert(out.faces.end(), {c0, c1, c2, c0, c2, c3}); else out.faces.insert(out.faces.end(), {c0, c3, c2, c0, c2, c1});
    }
    for (int a = 0; a < 3; ++a) for (int z = 0; z < Nz; ++z) for (int y = 0; y < Ny; ++y) for (int x = 0; x < Nx; ++x) {
        const int n[3] = {x, y, z}, u = (a + 1) % 3, v = (a + 2) % 3;
        if (n[a] + 1 >= N[a]) continue;
        int nb[3] = {x, y, z}; nb[a] += 1;
        if ((sn(n) <= 0) == (sn(nb) <= 0)) continue;
        out.n_open += n[u] == 0 || n[u] == N[u] - 1 || n[v] == 0 || n[v] == N[v] - 1;
    }
    return out;
}

enum { BLOBS, EMPTY_AND_FULL, HOSTILE };
// short_by: 0 the default capacities, 1 capacities exactly the largest counts, 2 one vertex short, 3 one face short
static int run_iso(const char* name, int B, int Nx, int Ny, int Nz, float level, int kind, int short_by) {
    std::uniform_real_distribution<float> ud(-0.5f, 0.5f);
    const size_t nodes = (size_t)Nx * Ny * Nz;
    std::vector<float> c[3]; const int N[3] = {Nx, Ny, Nz};
    for (int a = 0; a < 3; ++a) { float x = -0.5f; for (int i = 0; i < N[a]; ++i) { c[a].push_back(x); x += (1.0f + 0.5f * (ud(rng) + 0.5f)) / N[a]; } }   // unequal steps
    std::vector<float> field((size_t)B * nodes);
    for (int b = 0; b < B; ++b) {
        const float ox = 0.2f * ud(rng), oy = 0.2f * ud(rng), oz = 0.2f * ud(rng), r = 0.25f + 0.1f * ud(rng);
        for (int z = 0; z < Nz; ++z) for (int y = 0; y < Ny; ++y) for (int x = 0; x < Nx; ++x) {
            const float px = c[0][x] - 0.1f - ox, py = c[1][y] - 0.15f - oy, pz = c[2][z] - 0.1f - oz;
            float v = sqrtf(px * px + py * py + pz * pz) - r + 0.05f * sinf(9 * px) * sinf(7 * py) + level;
            if (kind == EMPTY_AND_FULL && b == 0) v = level + 1.0f;
            if (kind == EMPTY_AND_FULL && b == 1) v = level - 1.0f;
            field[b * nodes + ((size_t)z * Ny + y) * Nx + x] = v;
        }
    }
    if (kind == HOSTILE) for (size_t i = 0; i < field.size(); i += 7) { const int k = rng() % 6; if (k == 0) field[i] = NAN; else if (k == 1) field[i] = INFINITY; else if (k == 2) field[i] = -INFINITY; }
    std::vector<Mesh64> want;
    int top_v = 1, top_f = 1;
    for (int b = 0; b < B; ++b) { want.push_back(nets64(&field[b * nodes], c, level, Nx, Ny, Nz)); top_v = std::max(top_v, (int)want[b].verts.size() / 3); top_f = std::max(top_f, (int)want[b].faces.size() / 3); }
    const int Nmax = std::max(Nx, std::max(Ny, Nz));
    const int max_verts = short_by == 0 ? 8 * Nmax * Nmax : top_v - (short_by == 2), max_faces = short_by == 0 ? 16 * Nmax * Nmax : top_f - (short_by == 3);
    float *d_f = alv(field), *d_x = alv(c[0]), *d_y = alv(c[1]), *d_z = alv(c[2]);
    const size_t bytes = vpn_isosurface_workspace(B, Nx, Ny, Nz);
    void* ws = al16(bytes);
    float* verts = al<float>((size_t)B * max_verts * 3); int32_t* faces = al<int32_t>((size_t)B * max_faces * 3); int32_t* counts = al<int32_t>((size_t)B * 4);
    bool ok = bytes > 0 && max_verts > 0 && max_faces > 0 &&
              vpn_isosurface(d_f, d_x, d_y, d_z, level, B, Nx, Ny, Nz, max_verts, max_faces, ws, bytes, verts, faces, counts, nullptr) == 0;
    double worst = 0; int wrong = 0, overflowed = 0, open = 0, total_v = 0;
    for (int b = 0; b < B && ok; ++b) {
        const int nv = (int)want[b].verts.size() / 3, nf = (int)want[b].faces.size() / 3, over = nv > max_verts || nf > max_faces;
        const int32_t* cn = counts + (size_t)b * 4;
        wrong += cn[0] != nv || cn[1] != nf || cn[2] != want[b].n_open || cn[3] != over;
        overflowed += over; open += want[b].n_open; total_v += nv;
        const int live_v = over ? 0 : nv, live_f = over ? 0 : nf;
        for (int i = 0; i < max_verts * 3; ++i) {
            const float got = verts[(size_t)b * max_verts * 3 + i];
            if (i < live_v * 3) worst = std::max(worst, fabs(got - want[b].verts[i])); else wrong += got != 0.0f;
        }
        for (int i = 0; i < max_faces * 3; ++i) wrong += faces[(size_t)b * max_faces * 3 + i] != (i < live_f * 3 ? want[b].faces[i] : 0);
    }
    ok = ok && wrong == 0 && worst <= 1e-6;
    printf("%-34s B %d (%3d,%3d,%3d) blocks %4d  verts %5d  open %4d  capacity %6d / %6d  overflowed %d  worst %.2e  wrong %d  %s\n", name, B, Nx, Ny, Nz,
           ((Nx - 1) * (Ny - 1) * (Nz - 1) + 255) / 256, total_v, open, max_verts, max_faces, overflowed, worst, wrong, ok ? "ok" : "FAILED");
    for (void* p : {(void*)d_f, (void*)d_x, (void*)d_y, (void*)d_z, ws, (void*)verts, (void*)faces, (void*)counts}) free(p);
    return !ok;
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    bad += run_field("field, shared queries", 2, 3, 300, true, false);
    bad += run_field("field, K = 1, Q = 1", 1, 1, 1, false, false);
    bad += run_field("field, two stagings", 2, 300, 257, false, false);
    bad += run_field("field, NaN / inf / zero extent", 3, 5, 70, false, true);
    bad += run_iso("nets, (5,4,3)", 1, 5, 4, 3, 0.0f, BLOBS, 0);
    bad += run_iso("nets, (2,2,2)", 2, 2, 2, 2, 0.0f, BLOBS, 0);
    bad += run_iso("nets, 12^3, six blocks", 3, 12, 12, 12, 0.0f, BLOBS, 0);
    bad += run_iso("nets, (13,9,11), level 0.3", 2, 13, 9, 11, 0.3f, BLOBS, 0);
    bad += run_iso("nets, empty and all-inside", 3, 9, 8, 7, 0.0f, EMPTY_AND_FULL, 0);
    bad += run_iso("nets, NaN / inf nodes", 2, 11, 10, 9, -0.1f, HOSTILE, 0);
    bad += run_iso("nets, capacity = counts", 2, 10, 11, 9, 0.0f, BLOBS, 1);
    bad += run_iso("nets, one vertex short", 2, 10, 11, 9, 0.0f, BLOBS, 2);
    bad += run_iso("nets, one face short", 2, 10, 11, 9, 0.0f, BLOBS, 3);
    bad += run_iso("nets, 42^3, 270 blocks", 1, 42, 42, 42, 0.0f, BLOBS, 0);
    {   // validation without a launch
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int32_t i4[4] = {0, 0, 0, 0}; alignas(16) double st[512];
        const int big = VPN_OCCUPANCY_MAX_ITEMS + 1;
        auto fld = [&](int null_at, int B, int K, int Q) { const void* p[4] = {v, i4, v, v}; if (null_at >= 0) p[null_at] = nullptr;
            return vpn_primitive_field((const float*)p[0], (const int32_t*)p[1], (const float*)p[2], 1, B, K, Q, (float*)p[3], nullptr); };
        bool ok = true;
        for (int k = 0; k < 4; ++k) ok = ok && fld(k, 1, 1, 1) == VPN_E_BADARG;
        ok = ok && fld(-1, 0, 1, 1) == VPN_E_BADARG && fld(-1, 1, 0, 1) == VPN_E_BADARG && fld(-1, 1, 1, 0) == VPN_E_BADARG;
        ok = ok && fld(-1, 65536, 1, 1) == VPN_E_TOOBIG && fld(-1, 1, VPN_MAX_PRIMS + 1, 1) == VPN_E_TOOBIG && fld(-1, 1, 1, big) == VPN_E_TOOBIG;
        auto iso = [&](int null_at, float level, int B, int Nx, int Ny, int Nz, int mv, int mf, void* ws, size_t bytes) { const void* p[8] = {v, v, v, v, ws, v, i4, i4}; if (null_at >= 0) p[null_at] = nullptr;
            return vpn_isosurface((const float*)p[0], (const float*)p[1], (const float*)p[2], (const float*)p[3], level, B, Nx, Ny, Nz, mv, mf, (void*)p[4], bytes, (float*)p[5], (int32_t*)p[6], (int32_t*)p[7], nullptr); };
        const size_t need = vpn_isosurface_workspace(1, 2, 2, 2);
        ok = ok && need == 32;                                                  // one row of four ints, one table entry, rounded up to 16 bytes
        for (int k = 0; k < 8; ++k) ok = ok && iso(k, 0.0f, 1, 2, 2, 2, 1, 1, st, 4096) == VPN_E_BADARG;
        ok = ok && iso(-1, NAN, 1, 2, 2, 2, 1, 1, st, 4096) == VPN_E_BADARG && iso(-1, INFINITY, 1, 2, 2, 2, 1, 1, st, 4096) == VPN_E_BADARG;
        ok = ok && iso(-1, 0.0f, 0, 2, 2, 2, 1, 1, st, 4096) == VPN_E_BADARG && iso(-1, 0.0f, 1, 1, 2, 2, 1, 1, st, 4096) == VPN_E_BADARG &&
             iso(-1, 0.0f, 1, 2, 1, 2, 1, 1, st, 4096) == VPN_E_BADARG && iso(-1, 0.0f, 1, 2, 2, 0, 1, 1, st, 4096) == VPN_E_BADARG;
        ok = ok && iso(-1, 0.0f, 1, 2, 2, 2, 0, 1, st, 4096) == VPN_E_BADARG && iso(-1, 0.0f, 1, 2, 2, 2, 1, -1, st, 4096) == VPN_E_BADARG;
        ok = ok && iso(-1, 0.0f, 1, 2, 2, 2, 1, 1, st, need - 1) == VPN_E_BADARG && iso(-1, 0.0f, 1, 2, 2, 2, 1, 1, (char*)st + 8, 4088) == VPN_E_BADARG;
        ok = ok && iso(-1, 0.0f, 65536, 2, 2, 2, 1, 1, st, 4096) == VPN_E_TOOBIG && iso(-1, 0.0f, 1, 4097, 4096, 2, 1, 1, st, 4096) == VPN_E_TOOBIG &&
             iso(-1, 0.0f, 1, 2, 2, big / 4 + 1, 1, 1, st, 4096) == VPN_E_TOOBIG && iso(-1, 0.0f, 1, 65536, 65536, 65536, 1, 1, st, 4096) == VPN_E_TOOBIG;
        ok = ok && iso(-1, 0.0f, 1, 2, 2, 2, big, 1, st, 4096) == VPN_E_TOOBIG && iso(-1, 0.0f, 1, 2, 2, 2, 1, big, st, 4096) == VPN_E_TOOBIG;
        ok = ok && vpn_isosurface_workspace(0, 2, 2, 2) == 0 && vpn_isosurface_workspace(1, 1, 2, 2) == 0 && vpn_isosurface_workspace(1, 2, 2, big) == 0 &&
             vpn_isosurface_workspace(65536, 2, 2, 2) == 0 && vpn_isosurface_workspace(3, 42, 42, 42) == ((size_t)3 * (270 * 16 + 68921 * 4) + 15) / 16 * 16;
        printf("%-99s %s\n", "argument validation, workspace sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf("%.0f s of wall time\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
