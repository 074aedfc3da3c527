// Host check of the point-to-surface distance (csrc/pointmesh.hip) without a GPU, in the manner of
// tools/meshreg_host: the kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers) and compared with float64: the two means and the
// per-query distances against a double statement of the definitions, every index by the double distance of the pair it names,
// both gradients against central differences of that statement.  Checked: a tetrahedron (P = 1 and 65), the irregular mesh
// (a triple face, a face with a repeated index, a vertex in no face), a fan of 70 faces (two passes of a slice), a strip of
// 128 faces (P = 63), a closed 8 x 16 sphere at B = 2, P = 257 (two point tiles, two face slices, a pass of 62); each of
// dpoints / dverts alone; NaN and inf coordinates (every index stays in range, nothing is read past an end); the argument
// validation.  Every buffer has its exact size, so AddressSanitizer sees any access past an end.  It checks indexing, barriers
// and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/pointmesh_host/main.cpp -o pointmesh_host
//   ./pointmesh_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
// the two wave intrinsics the shim lacks: every lane publishes its predicate through the wave's exchange buffer
inline unsigned long long __ballot(int pred) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = pred ? 1.0f : 0.0f; g_wave[w].wait();
    unsigned long long m = 0;
    for (int k = 0; k < 64; ++k) if (g_xch[w][k] != 0.0f) m |= 1ull << k;
    g_wave[w].wait(); return m;
}
inline int __ffsll(unsigned long long x) { return __builtin_ffsll((long long)x); }
#include "../../volumetric-primitives-net_amd/csrc/pointmesh.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <array>
#include <chrono>
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(27);
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
template <class T> static T* alv(const std::vector<T>& v) { T* p = al<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

typedef std::array<int, 3> Face;
struct Mesh { std::vector<Face> faces; int n; };

// ---- the definitions in double
static double seg64(const double* p, const double* a, const double* b) {
    double ab[3], ap[3], l = 0, t = 0;
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ap[k] = p[k] - a[k]; l += ab[k] * ab[k]; t += ab[k] * ap[k]; }
    t = l > 0 ? std::min(1.0, std::max(0.0, t / l)) : 0.0;
    double q = 0;
    for (int k = 0; k < 3; ++k) { const double r = ap[k] - t * ab[k]; q += r * r; }
    return q;
}
static double pair64(const double* p, const double* v0, const double* v1, const double* v2) {
    double e1[3], e2[3], d[3], a = 0, b = 0, c = 0, d1 = 0, d2 = 0;
    for (int k = 0; k < 3; ++k) { e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k]; d[k] = p[k] - v0[k]; }
    for (int k = 0; k < 3; ++k) { a += e1[k] * e1[k]; b += e1[k] * e2[k]; c += e2[k] * e2[k]; d1 += e1[k] * d[k]; d2 += e2[k] * d[k]; }
    double best = INFINITY;
    const double det = a * c - b * b;
    if (det > 0) {
        const double s = (c * d1 - b * d2) / det, t = (a * d2 - b * d1) / det;
        if (s >= 0 && t >= 0 && s + t <= 1) { best = 0; for (int k = 0; k < 3; ++k) { const double r = d[k] - s * e1[k] - t * e2[k]; best += r * r; } }
    }
    return std::min(std::min(best, seg64(p, v0, v1)), std::min(seg64(p, v1, v2), seg64(p, v0, v2)));
}
struct Ref { std::vector<double> dp, df; double out[2]; };
// sample b alone (only = b >= 0) or the whole batch; the means are always over the whole batch's counts
static Ref values64(const Mesh& m, int B, int P, const std::vector<double>& pts, const std::vector<double>& v, int only = -1) {
    const int F = (int)m.faces.size();
    Ref r; r.dp.assign((size_t)B * P, INFINITY); r.df.assign((size_t)B * F, INFINITY); r.out[0] = r.out[1] = 0;
    for (int b = 0; b < B; ++b) {
        if (only >= 0 && b != only) continue;
        const double* vb = v.data() + (size_t)b * m.n * 3;
        for (int i = 0; i < P; ++i) for (int f = 0; f < F; ++f) {
            const double q = pair64(pts.data() + ((size_t)b * P + i) * 3, vb + m.faces[f][0] * 3, vb + m.faces[f][1] * 3, vb + m.faces[f][2] * 3);
            r.dp[(size_t)b * P + i] = std::min(r.dp[(size_t)b * P + i], q); r.df[(size_t)b * F + f] = std::min(r.df[(size_t)b * F + f], q);
        }
        for (int i = 0; i < P; ++i) r.out[0] += r.dp[(size_t)b * P + i];
        for (int f = 0; f < F; ++f) r.out[1] += r.df[(size_t)b * F + f];
    }
    r.out[0] /= (double)B * P; r.out[1] /= (double)B * F;
    return r;
}

static double cmp(const float* got, const std::vector<double>& want) {
    double m = 1e-30, d = 0;
    for (size_t i = 0; i < want.size(); ++i) { m = std::max(m, fabs(want[i])); d = std::max(d, fabs(want[i] - (double)got[i])); }
    return d / m;
}

struct Got { std::vector<float> dp, df, dpoints, dverts; std::vector<int> fop, pof; float out[2]; };
static void incidence(const Mesh& m, std::vector<int>& ptr, std::vector<int>& vf) {
    std::vector<std::vector<int>> per(m.n);
    for (int f = 0; f < (int)m.faces.size(); ++f) for (int c = 0; c < 3; ++c) per[m.faces[f][c]].push_back(4 * f + c);
    ptr.assign(1, 0); vf.clear();
    for (int i = 0; i < m.n; ++i) { for (int x : per[i]) vf.push_back(x); ptr.push_back((int)vf.size()); }
}

// forward and backward through the C entries with exactly sized buffers
static int run_entries(const Mesh& m, int B, int P, const std::vector<float>& pts, const std::vector<float>& v, const float up[2], Got& g) {
    const int F = (int)m.faces.size(), V = m.n;
    std::vector<int> fl, ptr, vf;
    for (const Face& f : m.faces) for (int c : f) fl.push_back(c);
    incidence(m, ptr, vf);
    float *d_pts = alv(pts), *d_v = alv(v);
    int *d_f = alv(fl), *d_ptr = alv(ptr), *d_vf = alv(vf);
    const size_t wsb = vpn_pointmesh_workspace(B, P, V, F);
    if (!wsb) { puts("  workspace size 0"); return 1; }
    void* ws = malloc(wsb);
    float *dp = al<float>((size_t)B * P), *df = al<float>((size_t)B * F), *o = al<float>(2), *gr = al<float>(2);
    int *fop = al<int>((size_t)B * P), *pof = al<int>((size_t)B * F);
    float *dpoints = al<float>((size_t)B * P * 3), *dverts = al<float>((size_t)B * V * 3);
    memcpy(gr, up, 8);
    int rc = vpn_pointmesh_fwd(d_pts, d_v, d_f, B, P, V, F, ws, wsb, dp, fop, df, pof, o, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    for (size_t i = 0; i < (size_t)B * P; ++i) if (fop[i] < 0 || fop[i] >= F) { puts("  face_of_point out of range"); return 1; }
    for (size_t i = 0; i < (size_t)B * F; ++i) if (pof[i] < 0 || pof[i] >= P) { puts("  point_of_face out of range"); return 1; }
    rc = vpn_pointmesh_bwd(gr, d_pts, d_v, d_f, fop, pof, d_ptr, d_vf, B, P, V, F, ws, wsb, dpoints, dverts, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    g.dp.assign(dp, dp + (size_t)B * P); g.df.assign(df, df + (size_t)B * F); g.fop.assign(fop, fop + (size_t)B * P); g.pof.assign(pof, pof + (size_t)B * F);
    g.dpoints.assign(dpoints, dpoints + (size_t)B * P * 3); g.dverts.assign(dverts, dverts + (size_t)B * V * 3); memcpy(g.out, o, 8);
    // a forward that writes only the means gives the same means; each gradient alone is the same gradient
    float *o2 = al<float>(2), *dpoints2 = al<float>((size_t)B * P * 3), *dverts2 = al<float>((size_t)B * V * 3);
    rc = vpn_pointmesh_fwd(d_pts, d_v, d_f, B, P, V, F, ws, wsb, nullptr, nullptr, nullptr, nullptr, o2, nullptr);
    if (rc || memcmp(o, o2, 8)) { puts("  forward without per-query outputs differs"); return 1; }
    rc = vpn_pointmesh_bwd(gr, d_pts, d_v, d_f, fop, pof, nullptr, nullptr, B, P, V, F, nullptr, 0, dpoints2, nullptr, nullptr);
    if (rc || memcmp(dpoints, dpoints2, (size_t)B * P * 12)) { puts("  dpoints alone differs"); return 1; }
    rc = vpn_pointmesh_bwd(gr, d_pts, d_v, d_f, fop, pof, d_ptr, d_vf, B, P, V, F, ws, (size_t)B * F * 36, nullptr, dverts2, nullptr);
    if (rc || memcmp(dverts, dverts2, (size_t)B * V * 12)) { puts("  dverts alone differs"); return 1; }
    for (void* p : {(void*)d_pts, (void*)d_v, (void*)d_f, (void*)d_ptr, (void*)d_vf, ws, (void*)dp, (void*)df, (void*)o, (void*)gr, (void*)fop, (void*)pof,
                    (void*)dpoints, (void*)dverts, (void*)o2, (void*)dpoints2, (void*)dverts2}) free(p);
    return 0;
}

static int run_case(const char* name, const Mesh& m, int B, int P, const std::vector<float>& pts, const std::vector<float>& v, bool grad = true) {
    const int F = (int)m.faces.size(), V = m.n;
    const float up[2] = {0.3f, -2.0f};
    Got g;
    if (run_entries(m, B, P, pts, v, up, g)) { printf("%-16s FAILED\n", name); return 1; }
    std::vector<double> p64(pts.begin(), pts.end()), v64(v.begin(), v.end());
    const Ref want = values64(m, B, P, p64, v64);
    double worst_v = 0;
    for (int k = 0; k < 2; ++k) worst_v = std::max(worst_v, fabs(g.out[k] - want.out[k]) / std::max(fabs(want.out[k]), 1e-30));
    const double worst_q = std::max(cmp(g.dp.data(), want.dp), cmp(g.df.data(), want.df));
    double worst_i = 0;                                      // the double distance of the pair an index names, over the double minimum
    for (int b = 0; b < B; ++b) {
        const double* vb = v64.data() + (size_t)b * V * 3;
        double top_p = 1e-30, top_f = 1e-30;
        for (int i = 0; i < P; ++i) top_p = std::max(top_p, want.dp[(size_t)b * P + i]);
        for (int f = 0; f < F; ++f) top_f = std::max(top_f, want.df[(size_t)b * F + f]);
        for (int i = 0; i < P; ++i) {
            const Face& fc = m.faces[g.fop[(size_t)b * P + i]];
            worst_i = std::max(worst_i, (pair64(p64.data() + ((size_t)b * P + i) * 3, vb + fc[0] * 3, vb + fc[1] * 3, vb + fc[2] * 3) - want.dp[(size_t)b * P + i]) / top_p);
        }
        for (int f = 0; f < F; ++f) {
            const Face& fc = m.faces[f];
            worst_i = std::max(worst_i, (pair64(p64.data() + ((size_t)b * P + g.pof[(size_t)b * F + f]) * 3, vb + fc[0] * 3, vb + fc[1] * 3, vb + fc[2] * 3) - want.df[(size_t)b * F + f]) / top_f);
        }
    }
    double worst_gp = 0, worst_gv = 0;
    if (grad) {                                             // central differences of the double statement, sample by sample
        const double h = 1e-6;
        std::vector<double> gp(p64.size()), gv(v64.size());
        for (int which = 0; which < 2; ++which) {
            std::vector<double>& x = which ? v64 : p64;
            std::vector<double>& gd = which ? gv : gp;
            const size_t per = x.size() / B;
            for (size_t i = 0; i < x.size(); ++i) {
                const double keep = x[i];
                x[i] = keep + h; const Ref hi = values64(m, B, P, p64, v64, (int)(i / per));
                x[i] = keep - h; const Ref lo = values64(m, B, P, p64, v64, (int)(i / per));
                x[i] = keep;
                gd[i] = (up[0] * (hi.out[0] - lo.out[0]) + up[1] * (hi.out[1] - lo.out[1])) / (2 * h);
            }
        }
        worst_gp = cmp(g.dpoints.data(), gp); worst_gv = cmp(g.dverts.data(), gv);
    }
    const bool ok = worst_v <= 1e-4 && worst_q <= 1e-4 && worst_i <= 1e-4 && worst_gp <= 1e-4 && worst_gv <= 1e-4;
    printf("%-16s B %d P %4d V %4d F %4d  means %.2e  distances %.2e  indices %.2e  dpoints %.2e  dverts %.2e  %s\n", name, B, P, V, F, worst_v,
           worst_q, worst_i, worst_gp, worst_gv, ok ? "ok" : "FAILED");
    return !ok;
}

static Mesh strip(int n) { Mesh m; m.n = n; for (int i = 0; i + 2 < n; ++i) m.faces.push_back(i % 2 == 0 ? Face{i, i + 1, i + 2} : Face{i + 1, i, i + 2}); return m; }
static Mesh fan(int val) { Mesh m; m.n = val + 1; for (int i = 0; i < val; ++i) m.faces.push_back({0, 1 + i, 1 + (i + 1) % val}); return m; }
static Mesh sphere(int rings, int seg) {
    Mesh m; m.n = rings * seg;
    for (int r = 0; r + 1 < rings; ++r) for (int s = 0; s < seg; ++s) {
        const int a = r * seg + s, b = r * seg + (s + 1) % seg, c = a + seg, d = b + seg;
        m.faces.push_back({a, c, b}); m.faces.push_back({b, c, d});
    }
    for (int s = 1; s + 1 < seg; ++s) { const int base = (rings - 1) * seg; m.faces.push_back({0, s, s + 1}); m.faces.push_back({base, base + s + 1, base + s}); }
    return m;
}

// a shape that belongs to the topology, moved per sample, plus a small random offset.  The tetrahedron is a regular one: with
// random corners a face can be a sliver, where the fp32 closest point is off by 25 ulp and more of the coordinates within the
// face's plane, which a point 2e-3 from it sees as 1e-3 of its gradient: the input's conditioning, not the kernels'
static std::vector<float> vertices(const char* kind, const Mesh& m, int B) {
    std::vector<float> v((size_t)B * m.n * 3);
    std::normal_distribution<float> nd(0, 1); std::uniform_real_distribution<float> ud(-0.5f, 0.5f);
    for (int b = 0; b < B; ++b) for (int i = 0; i < m.n; ++i) {
        float p[3];
        if (!strcmp(kind, "strip")) { p[0] = 0.05f * i; p[1] = 0.1f * (i % 2); p[2] = 0.03f * sinf(0.7f * i); }
        else if (!strcmp(kind, "fan")) { const float a = 6.2831853f * (i - 1) / (m.n - 1); p[0] = i ? 0.4f * cosf(a) : 0; p[1] = i ? 0.4f * sinf(a) : 0; p[2] = i ? 0.05f * cosf(3 * a) : 0.2f; }
        else if (!strcmp(kind, "sphere")) { const float th = 3.1415927f * (i / 16 + 0.5f) / 8, ph = 6.2831853f * (i % 16) / 16; p[0] = 0.3f * sinf(th) * cosf(ph); p[1] = 0.3f * cosf(th); p[2] = 0.3f * sinf(th) * sinf(ph); }
        else if (!strcmp(kind, "tet")) { p[0] = i < 2 ? 0.25f : -0.25f; p[1] = i % 2 ? -0.25f : 0.25f; p[2] = (i == 0 || i == 3) ? 0.25f : -0.25f; }
        else { p[0] = ud(rng); p[1] = ud(rng); p[2] = ud(rng); }
        for (int k = 0; k < 3; ++k) v[((size_t)b * m.n + i) * 3 + k] = p[k] * (1.0f + 0.2f * b) + 0.1f * b + 0.1f * tanhf(0.1f * nd(rng));
    }
    return v;
}
// barycentric samples on random faces, pushed off by 0.05 randn
static std::vector<float> cloud(const Mesh& m, const std::vector<float>& v, int B, int P) {
    std::vector<float> p((size_t)B * P * 3);
    std::uniform_real_distribution<float> ud(0, 1); std::normal_distribution<float> nd(0, 1);
    for (int b = 0; b < B; ++b) for (int i = 0; i < P; ++i) {
        const Face& f = m.faces[rng() % m.faces.size()];
        float w0 = ud(rng), w1 = ud(rng);
        if (w0 + w1 > 1) { w0 = 1 - w0; w1 = 1 - w1; }
        const float w[3] = {w0, w1, 1 - w0 - w1};
        for (int k = 0; k < 3; ++k) {
            float x = 0;
            for (int c = 0; c < 3; ++c) x += w[c] * v[((size_t)b * m.n + f[c]) * 3 + k];
            p[((size_t)b * P + i) * 3 + k] = x + 0.05f * nd(rng);
        }
    }
    return p;
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    Mesh tet{{{0, 1, 2}, {0, 2, 3}, {0, 3, 1}, {1, 3, 2}}, 4};
    Mesh irregular{{{0, 1, 2}, {1, 2, 0}, {0, 1, 2}, {2, 3, 5}, {3, 3, 4}, {4, 5, 6}, {6, 7, 0}, {5, 6, 7}}, 9};
    struct Case { const char* name; const char* kind; Mesh m; int B, P; };
    const std::vector<Case> cases = {{"tetrahedron", "tet", tet, 1, 1}, {"tetrahedron", "tet", tet, 1, 65}, {"irregular", "random", irregular, 1, 64},
                                     {"fan 70", "fan", fan(70), 1, 65}, {"strip 130", "strip", strip(130), 1, 63}, {"sphere 8 x 16", "sphere", sphere(8, 16), 2, 257}};
    for (const Case& c : cases) {
        const std::vector<float> v = vertices(c.kind, c.m, c.B);
        bad += run_case(c.name, c.m, c.B, c.P, cloud(c.m, v, c.B, c.P), v);
    }
    {   // degenerate faces, exact in both precisions (multiples of 1/4): a collinear face is its segment, three coincident
        // vertices are a point, a point on a face has distance 0
        Mesh m{{{0, 1, 2}, {3, 3, 3}, {0, 4, 5}}, 6};
        const std::vector<float> v = {0, 0, 0, 2, 0, 0, 1, 0, 0, 0, 0, 2, 0, 2, 0, 2, 2, 0}, pts = {1, 1, 1, 0, 0, 3, 0.5f, 1, 0, 3, 0, 0};
        const float up[2] = {1, 1};
        Got g;
        bool ok = !run_entries(m, 1, 4, pts, v, up, g);
        // point 0 (1,1,1): segment 2, point sqrt(1+1+1)^2 = 3, face 2 at height 1 -> 1 (face 2).  point 1 (0,0,3): point face 1: 1.
        // point 2 lies on face 2: 0.  point 3 (3,0,0): the segment's end (2,0,0): 1 (face 0)
        ok = ok && g.dp[0] == 1.0f && g.fop[0] == 2 && g.dp[1] == 1.0f && g.fop[1] == 1 && g.dp[2] == 0.0f && g.fop[2] == 2 && g.dp[3] == 1.0f && g.fop[3] == 0;
        ok = ok && g.df[0] == 1.0f && g.pof[0] == 2 && g.df[1] == 1.0f && g.pof[1] == 1 && g.df[2] == 0.0f && g.pof[2] == 2;
        for (float f : g.dpoints) ok = ok && std::isfinite(f);
        for (float f : g.dverts) ok = ok && std::isfinite(f);
        // point 2 lies on face 2 (its own record and that face's add exactly 0) and is the nearest of face 0, one above it
        ok = ok && g.dpoints[6] == 0.0f && fabs(g.dpoints[7] - 2.0 / 3) < 1e-6 && g.dpoints[8] == 0.0f;
        // point 1 is one above the point face 1: chosen by itself (2 / 4) and by that face (2 / 3)
        ok = ok && g.dpoints[3] == 0.0f && g.dpoints[4] == 0.0f && fabs(g.dpoints[5] - (0.5 + 2.0 / 3)) < 1e-6;
        printf("%-99s %s\n", "degenerate faces: the segment's and the point's distance, finite gradients, 0 on the surface", ok ? "ok" : "FAILED"); bad += !ok;
    }
    {   // NaN and inf coordinates: every index stays in range (run_entries checks), nothing is read past an end
        const Mesh m = fan(70);
        std::vector<float> v = vertices("fan", m, 2), pts = cloud(m, v, 2, 65);
        pts[3] = NAN; pts[10] = INFINITY; pts[65 * 3 + 1] = -INFINITY; v[5] = NAN; v[(71 + 7) * 3] = INFINITY;
        for (int k = 0; k < 3; ++k) v[(71 + 9) * 3 + k] = NAN;
        const float up[2] = {1, 1};
        Got g;
        bool ok = !run_entries(m, 2, 65, pts, v, up, g);
        std::vector<float> all_nan(pts.size(), NAN);
        ok = ok && !run_entries(m, 2, 65, all_nan, v, up, g);
        for (int i : g.fop) ok = ok && i == 0;
        for (int i : g.pof) ok = ok && i == 0;
        printf("%-99s %s\n", "NaN and inf coordinates: indices in range, index 0 where nothing compares", ok ? "ok" : "FAILED"); bad += !ok;
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; int32_t i4[4] = {0, 0, 0, 0};
        const size_t big_ws = (size_t)1 << 40;
        auto fwd = [&](int B, int P, int V, int F, size_t wsb) { return vpn_pointmesh_fwd(v, v, i4, B, P, V, F, v, wsb, v, i4, v, i4, v, nullptr); };
        auto bwd = [&](int B, int P, int V, int F, size_t wsb) { return vpn_pointmesh_bwd(v, v, v, i4, i4, i4, i4, i4, B, P, V, F, v, wsb, v, v, nullptr); };
        const int big = VPN_POINTMESH_MAX_ITEMS + 1;
        bool ok = vpn_pointmesh_fwd(nullptr, v, i4, 1, 4, 4, 4, v, big_ws, v, i4, v, i4, v, nullptr) == VPN_E_BADARG &&
                  vpn_pointmesh_fwd(v, nullptr, i4, 1, 4, 4, 4, v, big_ws, v, i4, v, i4, v, nullptr) == VPN_E_BADARG &&
                  vpn_pointmesh_fwd(v, v, nullptr, 1, 4, 4, 4, v, big_ws, v, i4, v, i4, v, nullptr) == VPN_E_BADARG &&
                  vpn_pointmesh_fwd(v, v, i4, 1, 4, 4, 4, nullptr, big_ws, v, i4, v, i4, v, nullptr) == VPN_E_BADARG &&
                  vpn_pointmesh_bwd(nullptr, v, v, i4, i4, i4, i4, i4, 1, 4, 4, 4, v, big_ws, v, v, nullptr) == VPN_E_BADARG &&
                  vpn_pointmesh_bwd(v, v, v, i4, nullptr, i4, i4, i4, 1, 4, 4, 4, v, big_ws, v, v, nullptr) == VPN_E_BADARG &&
                  vpn_pointmesh_bwd(v, v, v, i4, i4, i4, nullptr, i4, 1, 4, 4, 4, v, big_ws, v, v, nullptr) == VPN_E_BADARG &&      // dverts without the table
                  vpn_pointmesh_bwd(v, v, v, i4, i4, i4, i4, i4, 1, 4, 4, 4, nullptr, big_ws, nullptr, v, nullptr) == VPN_E_BADARG; // dverts without workspace
        // B = 8, P = V = 2048, F = 4032: 8 tiles, 16 slices of 252 faces, 16 chunks
        ok = ok && vpn_pointmesh_workspace(8, 2048, 2048, 4032) == 4 * ((size_t)8 * 4032 * 16 + (size_t)8 * 16 * 2048 * 2 + (size_t)8 * 8 * 4032 * 2 + 8 * 16 * 2) &&
             vpn_pointmesh_workspace(0, 4, 4, 4) == 0 && vpn_pointmesh_workspace(1, big, 4, 4) == 0;
        const size_t need = vpn_pointmesh_workspace(1, 4, 4, 4);
        ok = ok && fwd(1, 4, 4, 4, need - 1) == VPN_E_BADARG && bwd(1, 4, 4, 4, 4 * 36 - 1) == VPN_E_BADARG;
        for (int which = 0; which < 2; ++which) {
            auto call = [&](int B, int P, int V, int F) { return which ? bwd(B, P, V, F, big_ws) : fwd(B, P, V, F, big_ws); };
            ok = ok && call(0, 4, 4, 4) == VPN_E_BADARG && call(1, 0, 4, 4) == VPN_E_BADARG && call(1, 4, 0, 4) == VPN_E_BADARG && call(1, 4, 4, 0) == VPN_E_BADARG &&
                 call(-1, 4, 4, 4) == VPN_E_BADARG && call(65536, 4, 4, 4) == VPN_E_TOOBIG && call(1, big, 4, 4) == VPN_E_TOOBIG &&
                 call(1, 4, big, 4) == VPN_E_TOOBIG && call(1, 4, 4, big) == VPN_E_TOOBIG;
        }
        printf("%-99s %s\n", "argument validation and workspace sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf("%.0f s of wall time\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
