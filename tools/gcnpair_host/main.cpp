// Host check of the GCN's collapsed layer pairs (csrc/gcnpair.hip) without a GPU, in the manner of
// tools/gcnfactor_host: the kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers) and compared with float64.  Checked:
// vpn_gcn_aggregate2 forward (u, bias, ReLU present or absent) and as the masked backward with the partial sums of the
// intermediate, on a graph of disjoint strips whose blocks have 1, 3, 9 and 128 rows (each its own block, and merged
// greedily) and on a 60-vertex clique (more entries than a block stages in LDS), at C = 3 (element path) and C = 260
// (dwordx4 path with a 4-channel tail chunk); vpn_gcn_project_fwd / _bwd at Ci = 65 (element loads) and Ci = 64, R = 70 and 130 (a last chunk of 6 and of 2 rows), each gradient alone as well; the
// argument validation.  Every buffer has its exact size, so AddressSanitizer sees any access past an end.  It checks
// indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/gcnpair_host/main.cpp -o gcnpair_host
//   ./gcnpair_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
#include "../../volumetric-primitives-net_amd/csrc/gcnpair.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(11);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
static float* alf(const std::vector<float>& v) { float* p = al<float>(v.size()); memcpy(p, v.data(), v.size() * 4); return p; }

static double cmp(const float* got, const std::vector<double>& want) {
    double m = 1e-30, d = 0;
    for (size_t i = 0; i < want.size(); ++i) { m = std::max(m, fabs(want[i])); d = std::max(d, fabs(want[i] - (double)got[i])); }
    return d / m;
}

// disjoint strips (a path with chords up to `reach` apart) of the given sizes on consecutive indices: CSR of D^-1/2 (A + I) D^-1/2
struct Graph { int N; std::vector<int> rp, col, starts; std::vector<float> w; };
static Graph strips(const std::vector<int>& sizes, int reach = 2) {
    Graph g; g.N = 0; g.starts.push_back(0);
    std::vector<std::vector<int>> adj;
    for (int s : sizes) {
        for (int i = 0; i < s; ++i) adj.push_back({g.N + i});
        for (int i = 0; i < s; ++i) for (int d = 1; d <= reach; ++d) if (i + d < s) { adj[g.N + i].push_back(g.N + i + d); adj[g.N + i + d].push_back(g.N + i); }
        g.N += s; g.starts.push_back(g.N);
    }
    g.rp.push_back(0);
    for (int i = 0; i < g.N; ++i) {
        std::sort(adj[i].begin(), adj[i].end());
        for (int j : adj[i]) { g.col.push_back(j); g.w.push_back((float)(1.0 / sqrt((double)adj[i].size() * (double)adj[j].size()))); }
        g.rp.push_back((int)g.col.size());
    }
    return g;
}

static void hop64(const Graph& g, int B, int C, const std::vector<double>& x, const double* add, std::vector<double>& y) {
    y.assign(x.size(), 0.0);
    for (int b = 0; b < B; ++b) for (int i = 0; i < g.N; ++i) for (int c = 0; c < C; ++c) {
        double s = 0;
        for (int e = g.rp[i]; e < g.rp[i + 1]; ++e) s += (double)g.w[e] * x[((size_t)b * g.N + g.col[e]) * C + c];
        y[((size_t)b * g.N + i) * C + c] = s + (add ? add[c] : 0.0);
    }
}

static int run_hop2(const Graph& g, const std::vector<int>& starts, int C, bool has_u, bool has_b, int relu, bool backward, const char* what) {
    const int B = 2, nb = (int)starts.size() - 1;
    const size_t n = (size_t)B * g.N * C;
    std::vector<float> h(n), mk(n), u(C), bias(C);
    for (float& f : h) f = rnd();
    for (float& f : mk) f = rnd();                       // a ReLU output stands in: about half of it <= 0
    for (float& f : u) f = rnd();
    for (float& f : bias) f = rnd();
    float *dh = alf(h), *dm = alf(mk), *du = alf(u), *db = alf(bias), *out = al<float>(n), *w = alf(g.w);
    int *rp = al<int>(g.rp.size()), *col = al<int>(g.col.size()), *bl = al<int>(starts.size());
    memcpy(rp, g.rp.data(), g.rp.size() * 4); memcpy(col, g.col.data(), g.col.size() * 4); memcpy(bl, starts.data(), starts.size() * 4);
    const size_t wsb = vpn_gcn_aggregate2_workspace(B, nb, C);
    if (wsb != (size_t)B * nb * C * 4) { puts("  workspace size"); return 1; }
    float* part = backward ? al<float>(wsb / 4) : nullptr;
    const int rc = vpn_gcn_aggregate2(dh, backward ? dm : nullptr, rp, col, w, bl, nb, has_u ? du : nullptr, has_b ? db : nullptr, B, g.N, C, relu,
                                      out, part, nullptr);
    if (rc) { printf("  rc %d\n", rc); return 1; }
    std::vector<double> x(n), t, y, ud(u.begin(), u.end()), bd(bias.begin(), bias.end());
    for (size_t i = 0; i < n; ++i) x[i] = (backward && !(mk[i] > 0.0f)) ? 0.0 : (double)h[i];
    hop64(g, B, C, x, has_u ? ud.data() : nullptr, t);
    hop64(g, B, C, t, has_b ? bd.data() : nullptr, y);
    if (relu) for (double& v : y) v = std::max(v, 0.0);
    double worst = cmp(out, y);
    if (backward) {
        std::vector<double> want(C, 0.0); std::vector<float> got(C);
        for (size_t r = 0; r < (size_t)B * g.N; ++r) for (int c = 0; c < C; ++c) want[c] += t[r * C + c];
        for (int c = 0; c < C; ++c) { double s = 0; for (int p = 0; p < B * nb; ++p) s += (double)part[(size_t)p * C + c]; got[c] = (float)s; }
        worst = std::max(worst, cmp(got.data(), want));
    }
    const bool ok = worst <= 2e-5;
    printf("aggregate2  N %3d blocks %2d C %3d u %d b %d relu %d %-9s %-28s worst rel err %.2e  %s\n", g.N, nb, C, has_u, has_b, relu,
           backward ? "backward" : "forward", what, worst, ok ? "ok" : "FAILED");
    return !ok;
}

static int run_project(int R, int Ci, int Co) {
    std::vector<float> x((size_t)R * Ci), th((size_t)Ci * Co), g((size_t)R * Co);
    for (float& f : x) f = rnd();
    for (float& f : th) f = rnd();
    for (float& f : g) f = rnd();
    float *dx_in = alf(x), *dth = alf(th), *dg = alf(g), *out = al<float>((size_t)R * Co);
    int rc = vpn_gcn_project_fwd(dx_in, dth, R, Ci, Co, out, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    std::vector<double> o64((size_t)R * Co, 0.0), dx64((size_t)R * Ci, 0.0), dt64((size_t)Ci * Co, 0.0);
    for (int r = 0; r < R; ++r) for (int k = 0; k < Ci; ++k) for (int o = 0; o < Co; ++o) {
        o64[(size_t)r * Co + o] += (double)x[(size_t)r * Ci + k] * th[(size_t)k * Co + o];
        dx64[(size_t)r * Ci + k] += (double)g[(size_t)r * Co + o] * th[(size_t)k * Co + o];
        dt64[(size_t)k * Co + o] += (double)x[(size_t)r * Ci + k] * g[(size_t)r * Co + o];
    }
    double worst = cmp(out, o64);
    const size_t wsb = vpn_gcn_project_bwd_workspace(R, Ci, Co);
    if (wsb != (size_t)((R + 63) / 64) * Ci * Co * 4) { puts("  workspace size"); return 1; }
    void* ws = malloc(wsb);
    float *gx = al<float>((size_t)R * Ci), *gt = al<float>((size_t)Ci * Co);
    rc = vpn_gcn_project_bwd(dg, dx_in, dth, R, Ci, Co, ws, gx, gt, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    worst = std::max(worst, std::max(cmp(gx, dx64), cmp(gt, dt64)));
    int bad = 0;
    float *gx2 = al<float>((size_t)R * Ci), *gt2 = al<float>((size_t)Ci * Co);
    if (vpn_gcn_project_bwd(dg, nullptr, dth, R, Ci, Co, nullptr, gx2, nullptr, nullptr) || memcmp(gx, gx2, (size_t)R * Ci * 4)) { puts("  dx alone differs"); ++bad; }
    if (vpn_gcn_project_bwd(dg, dx_in, nullptr, R, Ci, Co, ws, nullptr, gt2, nullptr) || memcmp(gt, gt2, (size_t)Ci * Co * 4)) { puts("  dtheta alone differs"); ++bad; }
    const bool ok = !bad && worst <= 2e-5;
    printf("project     R %3d Ci %3d Co %d %61s worst rel err %.2e  %s\n", R, Ci, Co, "", worst, ok ? "ok" : "FAILED");
    return !ok;
}

int main() {
    int bad = 0;
    const Graph g = strips({1, 3, 9, 128, 9, 3, 1});
    std::vector<int> merged = {0};                       // greedy, left to right, at most 128 rows
    for (size_t i = 1; i < g.starts.size(); ++i) {
        if (i + 1 < g.starts.size() && g.starts[i + 1] - merged.back() <= GCN_HOP2_MAX_ROWS) continue;
        merged.push_back(g.starts[i]);
    }
    for (int C : {3, 260}) {
        bad += run_hop2(g, g.starts, C, true, true, 1, false, "a block a strip");
        bad += run_hop2(g, merged, C, true, true, 0, false, "strips merged up to 128");
        bad += run_hop2(g, g.starts, C, false, false, 0, false, "a block a strip");
        bad += run_hop2(g, merged, C, false, false, 0, true, "masked, partial sums");
        bad += run_hop2(g, g.starts, C, false, false, 0, true, "masked, partial sums");
    }
    const Graph dense = strips({60, 5}, 59);             // a clique of 60: 3600 entries, more than a block stages in LDS
    for (int C : {3, 260}) {
        bad += run_hop2(dense, dense.starts, C, true, true, 1, false, "a clique: entries from memory");
        bad += run_hop2(dense, dense.starts, C, false, false, 0, true, "a clique, masked, partial sums");
    }
    bad += run_project(70, 65, 3);
    bad += run_project(70, 64, 4);
    bad += run_project(130, 65, 1);
    bad += run_project(130, 8, 2);
    {   // validation without a launch
        alignas(16) float v[4] = {0, 0, 0, 0}; int32_t i4[4] = {0, 1, 0, 0};
        const int ok = vpn_gcn_aggregate2(nullptr, nullptr, i4, i4, v, i4, 1, nullptr, nullptr, 1, 1, 1, 0, v, nullptr, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_aggregate2(v, nullptr, i4, i4, v, nullptr, 1, nullptr, nullptr, 1, 1, 1, 0, v, nullptr, nullptr) == VPN_E_BADARG &&      // no table
                       vpn_gcn_aggregate2(v, nullptr, i4, i4, v, i4, 0, nullptr, nullptr, 1, 1, 1, 0, v, nullptr, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_aggregate2(v, nullptr, i4, i4, v, i4, 2, nullptr, nullptr, 1, 1, 1, 0, v, nullptr, nullptr) == VPN_E_BADARG &&           // more blocks than rows
                       vpn_gcn_aggregate2(v, nullptr, i4, i4, v, i4, 1, nullptr, nullptr, 0, 1, 1, 0, v, nullptr, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_aggregate2_workspace(2, 3, 5) == 2 * 3 * 5 * 4 && vpn_gcn_aggregate2_workspace(2, 0, 5) == 0 &&
                       vpn_gcn_project_fwd(v, v, 1, 4, 5, v, nullptr) == VPN_E_BADARG &&                                                                // Co
                       vpn_gcn_project_fwd(v, v, 1, 1025, 1, v, nullptr) == VPN_E_BADARG &&                                                             // Ci
                       vpn_gcn_project_fwd(v, nullptr, 1, 4, 1, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_project_bwd(nullptr, v, v, 1, 4, 1, v, v, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_project_bwd(v, v, v, 1, 4, 1, nullptr, nullptr, v, nullptr) == VPN_E_BADARG &&                                           // dtheta without workspace
                       vpn_gcn_project_bwd(v, v, nullptr, 1, 4, 1, v, v, nullptr, nullptr) == VPN_E_BADARG &&                                           // dx without theta
                       vpn_gcn_project_bwd(v, nullptr, nullptr, 1, 4, 1, nullptr, nullptr, nullptr, nullptr) == 0 &&
                       vpn_gcn_project_bwd_workspace(130, 8, 2) == 3 * 8 * 2 * 4 && vpn_gcn_project_bwd_workspace(130, 8, 5) == 0;
        printf("%-99s %s\n", "argument validation and workspace sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
