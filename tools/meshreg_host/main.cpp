// Host check of the mesh regularisers (csrc/meshreg.hip) without a GPU, in the manner of tools/gcnpair_host:
// the kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs workgroup by workgroup on
// std::threads, one per work-item, real barriers) and compared with float64: the three values against a double statement
// of the definitions, the gradient against central differences of that statement.  The tables are built here by plain
// loops (a third time, next to ops.mesh_topology and tests/meshreg_ref.py).  Checked: a tetrahedron, the same with one face
// flipped, an open strip of 7, 65 and 130 vertices (a wave and a forward chunk are crossed), the irregular mesh (a triple
// face, a face with a repeated index, a vertex in no face), a fan of valence 70, a closed 8 x 16 sphere and two disjoint
// components, at B = 1 and 3, l0 = 0 and 0.05, all terms and each alone, upstream gradient (0.3, -2, 5); degenerate
// geometry; the argument validation.  Every buffer has its exact size, so AddressSanitizer sees any access past an end.  It
// checks indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/meshreg_host/main.cpp -o meshreg_host
//   ./meshreg_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
#include "../../volumetric-primitives-net_amd/csrc/meshreg.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <array>
#include <cstdio>
#include <map>
#include <random>
#include <set>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(26);
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
template <class T> static T* alv(const std::vector<T>& v) { T* p = al<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

typedef std::array<int, 3> Face;
struct Mesh { std::vector<Face> faces; int n; };
struct Pair { int f, g, s; };
struct Topo {
    int n, E, F, P;
    std::vector<int> faces, edges, nbr_ptr, nbr, adj, vf_ptr, vf;
    std::vector<Pair> pairs;
};

static Topo topology(const Mesh& m) {
    Topo t; t.n = m.n; t.F = (int)m.faces.size();
    std::set<std::pair<int, int>> edges;
    std::map<std::pair<int, int>, std::vector<std::array<int, 3>>> inc;        // edge -> (face, slot, a < b)
    for (int f = 0; f < t.F; ++f) {
        const Face& c = m.faces[f];
        const bool real = c[0] != c[1] && c[1] != c[2] && c[2] != c[0];
        for (int j = 0; j < 3; ++j) {
            const int a = c[j], b = c[(j + 1) % 3];
            t.faces.push_back(c[j]);
            if (a == b) continue;
            const auto e = std::make_pair(std::min(a, b), std::max(a, b));
            edges.insert(e);
            if (real) inc[e].push_back({f, j, a < b});
        }
    }
    t.E = (int)edges.size();
    std::vector<std::set<int>> nb(m.n);
    for (auto& e : edges) { t.edges.push_back(e.first); t.edges.push_back(e.second); nb[e.first].insert(e.second); nb[e.second].insert(e.first); }
    t.nbr_ptr.push_back(0);
    for (int i = 0; i < m.n; ++i) { for (int j : nb[i]) t.nbr.push_back(j); t.nbr_ptr.push_back((int)t.nbr.size()); }
    t.adj.assign((size_t)t.F * 3, -1);
    for (auto& kv : inc) {
        if (kv.second.size() != 2) continue;
        const auto &x = kv.second[0], &y = kv.second[1];
        const int s = x[2] != y[2] ? 1 : -1;
        t.pairs.push_back({x[0], y[0], s});
        t.adj[x[0] * 3 + x[1]] = 2 * y[0] + (s < 0);
        t.adj[y[0] * 3 + y[1]] = 2 * x[0] + (s < 0);
    }
    t.P = (int)t.pairs.size();
    std::vector<std::vector<int>> vf(m.n);
    for (int f = 0; f < t.F; ++f) {
        if (t.adj[f * 3] < 0 && t.adj[f * 3 + 1] < 0 && t.adj[f * 3 + 2] < 0) continue;
        for (int c = 0; c < 3; ++c) vf[m.faces[f][c]].push_back(4 * f + c);
    }
    t.vf_ptr.push_back(0);
    for (int i = 0; i < m.n; ++i) { for (int x : vf[i]) t.vf.push_back(x); t.vf_ptr.push_back((int)t.vf.size()); }
    return t;
}

// the definitions in double: out[3] of one batch
static void values64(const Topo& t, int B, const std::vector<double>& v, double l0, int terms, double out[3]) {
    out[0] = out[1] = out[2] = 0.0;
    for (int b = 0; b < B; ++b) {
        const double* p = v.data() + (size_t)b * t.n * 3;
        if ((terms & 1) && t.E) for (int e = 0; e < t.E; ++e) {
            double q = 0;
            for (int k = 0; k < 3; ++k) { const double d = p[t.edges[2 * e] * 3 + k] - p[t.edges[2 * e + 1] * 3 + k]; q += d * d; }
            out[0] += l0 == 0.0 ? q : (sqrt(q) - l0) * (sqrt(q) - l0);
        }
        if ((terms & 2) && t.E) for (int i = 0; i < t.n; ++i) {
            const int deg = t.nbr_ptr[i + 1] - t.nbr_ptr[i];
            if (!deg) continue;
            for (int k = 0; k < 3; ++k) {
                double s = 0;
                for (int e = t.nbr_ptr[i]; e < t.nbr_ptr[i + 1]; ++e) s += p[t.nbr[e] * 3 + k];
                const double d = s / deg - p[i * 3 + k];
                out[1] += d * d;
            }
        }
        if ((terms & 4) && t.P) for (const Pair& pr : t.pairs) {
            double n[2][3], len[2];
            for (int w = 0; w < 2; ++w) {
                const int f = w ? pr.g : pr.f;
                const double *a = p + t.faces[3 * f] * 3, *bb = p + t.faces[3 * f + 1] * 3, *c = p + t.faces[3 * f + 2] * 3;
                const double e1[3] = {bb[0] - a[0], bb[1] - a[1], bb[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                n[w][0] = e1[1] * e2[2] - e1[2] * e2[1]; n[w][1] = e1[2] * e2[0] - e1[0] * e2[2]; n[w][2] = e1[0] * e2[1] - e1[1] * e2[0];
                len[w] = std::max(sqrt(n[w][0] * n[w][0] + n[w][1] * n[w][1] + n[w][2] * n[w][2]), 1e-8);
            }
            out[2] += 1.0 - pr.s * (n[0][0] * n[1][0] + n[0][1] * n[1][1] + n[0][2] * n[1][2]) / (len[0] * len[1]);
        }
    }
    if ((terms & 1) && t.E) out[0] /= (double)B * t.E;
    if ((terms & 2) && t.E) out[1] /= (double)B * t.n;
    if ((terms & 4) && t.P) out[2] /= (double)B * t.P;
}

static double cmp(const float* got, const std::vector<double>& want) {
    double m = 1e-30, d = 0;
    for (size_t i = 0; i < want.size(); ++i) { m = std::max(m, fabs(want[i])); d = std::max(d, fabs(want[i] - (double)got[i])); }
    return d / m;
}

// runs forward and backward through the C entries with exactly sized buffers; returns values and gradient
static int run_entries(const Topo& t, int B, const std::vector<float>& v, float l0, int terms, const float up[3], float out[3], std::vector<float>& dv) {
    float* dverts_in = alv(v);
    int *faces = alv(t.faces), *edges = alv(t.edges), *nbr_ptr = alv(t.nbr_ptr), *nbr = alv(t.nbr), *adj = alv(t.adj), *vf_ptr = alv(t.vf_ptr), *vf = alv(t.vf);
    const size_t wsb = vpn_meshreg_workspace(B, t.n, t.E, t.F);
    const int longest = std::max(t.n, std::max(t.E, t.F));
    if (wsb != (size_t)B * ((longest + 255) / 256) * 3 * 4) { puts("  workspace size"); return 1; }
    void* ws = malloc(wsb);
    float *delta = al<float>((size_t)B * t.n * 3), *normals = al<float>((size_t)B * t.F * 3), *o = al<float>(3), *g = al<float>(3);
    float* grad = al<float>((size_t)B * t.n * 3);
    memcpy(g, up, 12);
    int rc = vpn_meshreg_fwd(dverts_in, faces, edges, nbr_ptr, nbr, adj, B, t.n, t.E, t.F, t.P, l0, terms, ws, delta, normals, o, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    rc = vpn_meshreg_bwd(g, dverts_in, delta, normals, faces, nbr_ptr, nbr, vf_ptr, vf, adj, B, t.n, t.E, t.F, t.P, l0, terms, grad, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    memcpy(out, o, 12);
    dv.assign(grad, grad + (size_t)B * t.n * 3);
    // a forward that saves nothing gives the same values
    float* o2 = al<float>(3);
    rc = vpn_meshreg_fwd(dverts_in, faces, edges, nbr_ptr, nbr, adj, B, t.n, t.E, t.F, t.P, l0, terms, ws, nullptr, nullptr, o2, nullptr);
    if (rc || memcmp(o, o2, 12)) { puts("  forward without saved tensors differs"); return 1; }
    for (void* p : {(void*)dverts_in, (void*)faces, (void*)edges, (void*)nbr_ptr, (void*)nbr, (void*)adj, (void*)vf_ptr, (void*)vf, ws, (void*)delta,
                    (void*)normals, (void*)o, (void*)g, (void*)grad, (void*)o2}) free(p);
    return 0;
}

static int run_case(const char* name, const Mesh& m, const std::vector<float>& v, int B, float l0, int terms, double tol_grad = 1e-4) {
    const Topo t = topology(m);
    const float up[3] = {0.3f, -2.0f, 5.0f};
    float out[3]; std::vector<float> dv;
    if (run_entries(t, B, v, l0, terms, up, out, dv)) return 1;
    std::vector<double> x(v.begin(), v.end()), want(3), gd(x.size());
    values64(t, B, x, l0, terms, want.data());
    double worst_v = 0;
    for (int k = 0; k < 3; ++k) worst_v = std::max(worst_v, fabs(out[k] - want[k]) / std::max(fabs(want[k]), 1e-30) * (want[k] != 0.0 || out[k] != 0.0f));
    for (size_t i = 0; i < x.size(); ++i) {                 // central differences of the double statement
        const double keep = x[i], h = 1e-6;
        double hi[3], lo[3];
        x[i] = keep + h; values64(t, B, x, l0, terms, hi);
        x[i] = keep - h; values64(t, B, x, l0, terms, lo);
        x[i] = keep;
        gd[i] = 0;
        for (int k = 0; k < 3; ++k) gd[i] += up[k] * (hi[k] - lo[k]) / (2 * h);
    }
    double gmax = 0;
    for (double d : gd) gmax = std::max(gmax, fabs(d));
    const double worst_g = gmax > 0 ? cmp(dv.data(), gd) : 0.0;
    bool zero_ok = true;                                    // a term that is off gives exactly 0
    for (int k = 0; k < 3; ++k) if (!(terms & (1 << k)) && out[k] != 0.0f) zero_ok = false;
    const bool ok = worst_v <= 1e-4 && worst_g <= tol_grad && zero_ok;
    printf("%-20s V %4d E %4d F %4d P %4d B %d l0 %.2f terms %d  values %.2e  gradient %.2e  %s\n", name, t.n, t.E, t.F, t.P, B, l0, terms,
           worst_v, worst_g, ok ? "ok" : "FAILED");
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

// a shape that belongs to the topology (faces with area), moved per sample, plus a small random offset
static std::vector<float> vertices(const char* kind, const Mesh& m, int B) {
    std::vector<float> v((size_t)B * m.n * 3);
    std::normal_distribution<float> nd(0, 1); std::uniform_real_distribution<float> ud(-0.5f, 0.5f);
    for (int b = 0; b < B; ++b) for (int i = 0; i < m.n; ++i) {
        float p[3];
        if (!strcmp(kind, "strip")) { p[0] = 0.05f * i; p[1] = 0.1f * (i % 2); p[2] = 0.03f * sinf(0.7f * i); }
        else if (!strcmp(kind, "fan")) { const float a = 6.2831853f * (i - 1) / (m.n - 1); p[0] = i ? 0.4f * cosf(a) : 0; p[1] = i ? 0.4f * sinf(a) : 0; p[2] = i ? 0.05f * cosf(3 * a) : 0.2f; }
        else if (!strcmp(kind, "sphere")) { const float th = 3.1415927f * (i / 16 + 0.5f) / 8, ph = 6.2831853f * (i % 16) / 16; p[0] = 0.3f * sinf(th) * cosf(ph); p[1] = 0.3f * cosf(th); p[2] = 0.3f * sinf(th) * sinf(ph); }
        else { p[0] = ud(rng); p[1] = ud(rng); p[2] = ud(rng); }
        for (int k = 0; k < 3; ++k) v[((size_t)b * m.n + i) * 3 + k] = p[k] * (1.0f + 0.2f * b) + 0.1f * b + 0.1f * tanhf(0.1f * nd(rng));
    }
    return v;
}

int main() {
    int bad = 0;
    Mesh tet{{{0, 1, 2}, {0, 2, 3}, {0, 3, 1}, {1, 3, 2}}, 4}, flipped{{{0, 1, 2}, {0, 3, 2}, {0, 3, 1}, {1, 3, 2}}, 4};
    Mesh irregular{{{0, 1, 2}, {1, 2, 0}, {0, 1, 2}, {2, 3, 5}, {3, 3, 4}, {4, 5, 6}, {6, 7, 0}, {5, 6, 7}}, 9};
    Mesh two = tet; two.n = 9; for (const Face& f : strip(5).faces) two.faces.push_back({f[0] + 4, f[1] + 4, f[2] + 4});
    struct Case { const char* name; const char* kind; Mesh m; };
    const std::vector<Case> cases = {{"tetrahedron", "random", tet}, {"tetrahedron flipped", "random", flipped}, {"strip 7", "strip", strip(7)},
                                     {"irregular", "random", irregular}, {"fan 70", "fan", fan(70)}, {"sphere 8 x 16", "sphere", sphere(8, 16)},
                                     {"two components", "random", two}, {"strip 65", "strip", strip(65)}, {"strip 130", "strip", strip(130)}};
    for (const Case& c : cases) {
        {   // the tables say what the issue states of the named meshes
            const Topo t = topology(c.m);
            int flips = 0; for (const Pair& p : t.pairs) flips += p.s < 0;
            bool ok = true;
            if (!strcmp(c.name, "tetrahedron")) ok = t.E == 6 && t.P == 6 && flips == 0;
            if (!strcmp(c.name, "tetrahedron flipped")) ok = t.E == 6 && t.P == 6 && flips == 3;
            if (!strcmp(c.name, "sphere 8 x 16")) ok = t.E == 378 && t.F == 252 && t.P == 378 && flips == 0;
            if (!strcmp(c.name, "fan 70")) ok = t.nbr_ptr[1] == 70 && t.P == 70;
            if (!ok) { printf("%-20s topology FAILED\n", c.name); ++bad; }
        }
        for (int B : {1, 3}) {
            const std::vector<float> v = vertices(c.kind, c.m, B);
            for (float l0 : {0.0f, 0.05f}) {
                bad += run_case(c.name, c.m, v, B, l0, 7);
                if (B == 3) for (int terms : {1, 2, 4, 0}) bad += run_case(c.name, c.m, v, B, l0, terms);
            }
        }
    }
    {   // degenerate geometry: a zero-area face, a zero-length edge with l0 > 0, two coincident vertices.  Multiples of 1/4:
        // exact in both precisions.  The values are compared with the double statement; the gradient must be finite, and of
        // the edge and Laplacian terms (smooth here but at the zero-length edge, whose gradient is 0 by definition) equal it
        Mesh m{{{0, 1, 2}, {0, 2, 3}, {2, 1, 3}, {3, 4, 5}, {1, 4, 3}}, 6};
        const std::vector<float> v = {0, 0, 0, 1, 0, 0, 0.5f, 0, 0, 0.5f, 1, 0.25f, 1.5f, 1, 0, 1.5f, 1, 0};
        const Topo t = topology(m);
        const float up[3] = {1, 1, 1};
        float out[3]; std::vector<float> dv;
        bool ok = !run_entries(t, 1, v, 0.25f, 7, up, out, dv);
        std::vector<double> x(v.begin(), v.end()); double want[3];
        values64(t, 1, x, 0.25, 7, want);
        for (int k = 0; k < 3 && ok; ++k) ok = fabs(out[k] - want[k]) <= 1e-5 * fabs(want[k]);
        for (float f : dv) ok = ok && std::isfinite(f);
        printf("%-99s %s\n", "degenerate geometry: values equal the statement, the gradient is finite", ok ? "ok" : "FAILED"); bad += !ok;
        ok = !run_entries(t, 1, v, 0.25f, 1, up, out, dv);
        // vertex 5 touches 3 and 4 (length 0): only edge (3, 5) pulls it
        const double len = sqrt(1.0 + 0.0625), c = 2.0 / t.E * (1.0 - 0.25 / len);
        ok = ok && fabs(dv[15] - c * 1.0) < 1e-6 && fabs(dv[16]) < 1e-7 && fabs(dv[17] - c * -0.25) < 1e-6;
        printf("%-99s %s\n", "a zero-length edge with l0 > 0 pulls neither end", ok ? "ok" : "FAILED"); bad += !ok;
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; int32_t i4[4] = {0, 0, 0, 0};
        auto fwd = [&](int B, int V, int E, int F, int P, float l0, int terms) { return vpn_meshreg_fwd(v, i4, i4, i4, i4, i4, B, V, E, F, P, l0, terms, v, v, v, v, nullptr); };
        auto bwd = [&](int B, int V, int E, int F, int P, float l0, int terms) { return vpn_meshreg_bwd(v, v, v, v, i4, i4, i4, i4, i4, i4, B, V, E, F, P, l0, terms, v, nullptr); };
        const int big = VPN_MESHREG_MAX_ITEMS + 1;
        bool ok = vpn_meshreg_fwd(nullptr, i4, i4, i4, i4, i4, 1, 4, 6, 4, 6, 0, 7, v, v, v, v, nullptr) == VPN_E_BADARG &&
                  vpn_meshreg_fwd(v, i4, i4, i4, i4, i4, 1, 4, 6, 4, 6, 0, 7, nullptr, v, v, v, nullptr) == VPN_E_BADARG &&        // no workspace
                  vpn_meshreg_fwd(v, i4, nullptr, i4, i4, i4, 1, 4, 6, 4, 6, 0, 7, v, v, v, v, nullptr) == VPN_E_BADARG &&         // edges with E > 0
                  vpn_meshreg_bwd(nullptr, v, v, v, i4, i4, i4, i4, i4, i4, 1, 4, 6, 4, 6, 0, 7, v, nullptr) == VPN_E_BADARG &&
                  vpn_meshreg_bwd(v, v, nullptr, v, i4, i4, i4, i4, i4, i4, 1, 4, 6, 4, 6, 0, 2, v, nullptr) == VPN_E_BADARG &&     // lap without delta
                  vpn_meshreg_bwd(v, v, v, nullptr, i4, i4, i4, i4, i4, i4, 1, 4, 6, 4, 6, 0, 4, v, nullptr) == VPN_E_BADARG &&     // normal without normals
                  vpn_meshreg_workspace(8, 2048, 6048, 4032) == 8 * 24 * 3 * 4 && vpn_meshreg_workspace(0, 4, 6, 4) == 0;
        for (int which = 0; which < 2; ++which) {
            auto call = [&](int B, int V, int E, int F, int P, float l0, int terms) { return which ? bwd(B, V, E, F, P, l0, terms) : fwd(B, V, E, F, P, l0, terms); };
            ok = ok && call(0, 4, 6, 4, 6, 0, 7) == VPN_E_BADARG && call(1, 0, 6, 4, 6, 0, 7) == VPN_E_BADARG && call(1, 4, 6, 0, 6, 0, 7) == VPN_E_BADARG &&
                 call(1, 4, -1, 4, 6, 0, 7) == VPN_E_BADARG && call(1, 4, 6, 4, -1, 0, 7) == VPN_E_BADARG && call(1, 4, 6, 4, 6, 0, 8) == VPN_E_BADARG &&
                 call(1, 4, 6, 4, 6, -1.0f, 7) == VPN_E_BADARG && call(1, 4, 6, 4, 6, NAN, 7) == VPN_E_BADARG && call(1, 4, 6, 4, 6, INFINITY, 7) == VPN_E_BADARG &&
                 call(65536, 4, 6, 4, 6, 0, 7) == VPN_E_TOOBIG && call(1, big, 6, 4, 6, 0, 7) == VPN_E_TOOBIG && call(1, 4, big, 4, 6, 0, 7) == VPN_E_TOOBIG &&
                 call(1, 4, 6, big, 6, 0, 7) == VPN_E_TOOBIG;
        }
        printf("%-99s %s\n", "argument validation and workspace sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
