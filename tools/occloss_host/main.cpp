// Host check of the occupancy loss (csrc/occloss.hip) without a GPU, in the manner of tools/occupancy_host: the
// four kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs workgroup by workgroup on
// std::threads, one per work-item, real barriers) and compared with a double statement of the definition: the logit and the
// overlap sum per query, the two losses, the count of skipped queries, and the gradient against central differences of the
// double loss.  Inputs include Q and K that are no multiples of the tile, the slice and the staging, both label types, shared
// and per-sample queries, every slice size of the backward (the kernel is also launched directly with 2, 4 and 8 queries a
// lane), NaN / inf parameters, queries and labels, extents of 0; and every rejected argument.  Every buffer has its exact size,
// so AddressSanitizer sees any access past an end.  It checks indexing, barriers and the host-side launch logic; it says nothing
// about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/occloss_host/main.cpp -o occloss_host
//   ./occloss_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
#include "../../volumetric-primitives-net_amd/csrc/occloss.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <chrono>
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(31);
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
template <class T> static T* alv(const std::vector<T>& v) { T* p = al<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }
static void* al16(size_t bytes) { void* p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 16)) return nullptr; return p; }   // exact size, 16-byte aligned

// ---- the definition in double on given (double) parameters
static void rotation64(const double* q, double R[3][3]) {
    const double PI32 = 3.1415927410125732;
    const double r = q[3] - floor(q[3]), h = ((r * 2) * PI32) / 2;
    const double a = q[0] * sin(h), b = q[1] * sin(h), c = q[2] * sin(h), d = cos(h), l = sqrt(a * a + b * b + c * c + d * d);
    const double x = a / l, y = b / l, z = c / l, w = d / l;
    R[0][0] = x * x - y * y - z * z + w * w; R[0][1] = 2 * (x * y - z * w); R[0][2] = 2 * (x * z + y * w);
    R[1][0] = 2 * (x * y + z * w); R[1][1] = -x * x + y * y - z * z + w * w; R[1][2] = 2 * (y * z - x * w);
    R[2][0] = 2 * (x * z - y * w); R[2][1] = 2 * (y * z + x * w); R[2][2] = -x * x - y * y + z * z + w * w;
}
static double sigmoid64(double z) { const double e = exp(-fabs(z)); return (z >= 0 ? 1.0 : e) / (1 + e); }

struct Query64 { double l, s, bce, ov; bool skipped; };
// one sample: prm [K][10] double, R per primitive
static Query64 query64(const double* prm, const std::vector<double>& R, const int* kinds, int K, const float* x, double y, double tau) {
    double zmax = -INFINITY; std::vector<double> z(K, -INFINITY);
    Query64 r{-INFINITY, 0, 0, 0, false};
    for (int k = 0; k < K; ++k) {
        const double* p = prm + (size_t)k * 10; const double* Rk = &R[(size_t)k * 9];
        const double d[3] = {(double)x[0] - p[7], (double)x[1] - p[8], (double)x[2] - p[9]};
        double u[3];
        for (int i = 0; i < 3; ++i) u[i] = (Rk[i] * d[0] + Rk[3 + i] * d[1] + Rk[6 + i] * d[2]) / p[i];
        double m = NAN;
        if (!(std::isnan(u[0]) || std::isnan(u[1]) || std::isnan(u[2])))
            m = kinds[k] == VPN_SPHERE ? u[0] * u[0] + u[1] * u[1] + u[2] * u[2] : std::max(fabs(u[0]), std::max(fabs(u[1]), fabs(u[2])));
        if (!std::isfinite(m)) continue;
        z[k] = -(m - 1) / tau; zmax = std::max(zmax, z[k]); r.s += sigmoid64(z[k]);
    }
    if (std::isfinite(zmax)) { double t = 0; for (int k = 0; k < K; ++k) if (z[k] > -INFINITY) t += exp(z[k] - zmax); r.l = zmax + log(t); } else r.l = zmax;
    r.skipped = !(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2])) || std::isnan(y) || !std::isfinite(r.l);
    if (!r.skipped) { r.bce = std::max(r.l, 0.0) + log1p(exp(-fabs(r.l))) - y * r.l; const double o = r.s - 1; r.ov = o > 0 ? o * o : 0; }
    return r;
}
// sum over the queries of sample b of g0 bce + g1 ov (not yet divided)
static double sample64(const double* prm, const int* kinds, int K, const float* q, const double* y, int Q, double tau, double g0, double g1) {
    std::vector<double> R((size_t)K * 9);
    for (int k = 0; k < K; ++k) { double M[3][3]; rotation64(prm + (size_t)k * 10 + 3, M); for (int i = 0; i < 9; ++i) R[(size_t)k * 9 + i] = M[i / 3][i % 3]; }
    double t = 0;
    for (int i = 0; i < Q; ++i) { const Query64 r = query64(prm, R, kinds, K, q + (size_t)i * 3, y[i], tau); t += g0 * r.bce + g1 * r.ov; }
    return t;
}

// qpl 0: the entries as they plan; otherwise the backward's two kernels launched with qpl queries a lane
static int run(const char* name, int B, int K, int Q, bool shared, bool u8, float tau, bool hostile, int qpl) {
    std::uniform_real_distribution<float> ud(-0.5f, 0.5f), uv(0.08f, 0.3f);
    std::vector<float> params((size_t)B * K * 10), q((size_t)(shared ? 1 : B) * Q * 3), labf((size_t)B * Q);
    std::vector<uint8_t> lab8((size_t)B * Q);
    std::vector<int> kinds(K);
    for (int i = 0; i < B * K; ++i) { float* p = &params[(size_t)i * 10]; for (int k = 0; k < 3; ++k) p[k] = uv(rng); for (int k = 3; k < 6; ++k) p[k] = 2 * ud(rng); p[6] = 0.1f + 0.8f * (ud(rng) + 0.5f) + (float)(int)(rng() % 3) - 1.0f; for (int k = 7; k < 10; ++k) p[k] = 0.6f * ud(rng); }
    for (int& k : kinds) k = rng() % 2;
    for (float& x : q) x = ud(rng);
    for (size_t i = 0; i < labf.size(); ++i) { lab8[i] = rng() % 3 == 0 ? (uint8_t)(1 + rng() % 255) : 0; labf[i] = u8 ? (lab8[i] ? 1.0f : 0.0f) : (rng() % 4 ? (float)(rng() % 2) : ud(rng) + 0.5f); }
    std::vector<char> dead((size_t)B * K, 0);
    if (hostile) {
        q[0] = NAN; q[4] = INFINITY; if (!u8) labf[2] = NAN;
        params[0] = 0.0f; dead[0] = 1;                                            // an extent of 0
        if (K > 1) { params[10 + 1] = NAN; dead[1] = 1; }
        if (K > 2) { params[20 + 8] = INFINITY; dead[2] = 1; }
        params[(size_t)(B * K - 1) * 10 + 3] = INFINITY; dead[(size_t)B * K - 1] = 1;
        if (B > 1) for (int k = 0; k < K; ++k) { params[((size_t)(B - 2) * K + k) * 10 + 2] = 0.0f; dead[(size_t)(B - 2) * K + k] = 1; }   // a sample with nothing left
    }
    const float g[2] = {0.7f, 1.5f};
    float *d_p = alv(params), *d_q = alv(q), *d_g = alv(std::vector<float>(g, g + 2)); int* d_k = alv(kinds);
    void* d_l = u8 ? (void*)alv(lab8) : (void*)alv(labf);
    const size_t bytes = vpn_occloss_workspace(B, K, Q);
    void* ws = al16(bytes);
    float *lse = al<float>((size_t)B * Q), *s = al<float>((size_t)B * Q), *lse2 = al<float>((size_t)B * Q), *s2 = al<float>((size_t)B * Q), *out = al<float>(2), *dp = al<float>((size_t)B * K * 10);
    int32_t* skipped = al<int32_t>(1);
    bool ok = bytes > 0 && vpn_occloss_fwd(d_p, d_k, d_q, shared, d_l, u8, B, K, Q, tau, ws, bytes, lse, s, out, skipped, nullptr) == 0;
    ok = ok && vpn_occloss_fwd(d_p, d_k, d_q, shared, nullptr, 0, B, K, Q, tau, nullptr, 0, lse2, s2, nullptr, nullptr, nullptr) == 0;   // the soft occupancy alone
    ok = ok && !memcmp(lse, lse2, (size_t)B * Q * 4) && !memcmp(s, s2, (size_t)B * Q * 4);
    float out2[2]; ok = ok && vpn_occloss_fwd(d_p, d_k, d_q, shared, d_l, u8, B, K, Q, tau, ws, bytes, nullptr, nullptr, out2, nullptr, nullptr) == 0 && !memcmp(out, out2, 8);
    int slice = 0; const int slices = vpn_occloss_plan(B, Q, &slice);
    if (ok && qpl == 0) ok = vpn_occloss_bwd(d_g, d_p, d_k, d_q, shared, d_l, u8, lse, s, B, K, Q, tau, ws, bytes, dp, nullptr) == 0;
    void* ws2 = nullptr;
    if (ok && qpl > 0) {                    // the backward's kernels with another slice than the plan's: exactly sized partial sums
        const int sl = (Q + 256 * qpl - 1) / (256 * qpl);
        ws2 = al16((size_t)B * sl * 4 * K * 12 * sizeof(float));
        hipLaunchKernelGGL(occl_bwd_kernel, dim3(sl, B), dim3(256), 0, nullptr, (const float*)d_g, (const float*)d_p, (const int32_t*)d_k, (const float*)d_q,
                           shared ? 0LL : 3LL * Q, (const void*)d_l, (int)u8, (const float*)lse, (const float*)s, K, Q, qpl, sl, tau, (double)B * Q, (float*)ws2);
        hipLaunchKernelGGL(occl_bwd_finish_kernel, dim3((B * K + 3) / 4), dim3(64), 0, nullptr, (const float*)ws2, (const float*)d_p, B * K, K, 4 * sl, dp);
    }
    // the definition
    double want[2] = {0, 0}, worst_q = 0, worst_g = 0, gmax = 0; long long want_skipped = 0; int nonfinite = 0, dead_wrong = 0;
    std::vector<double> grad((size_t)B * K * 10, 0.0);
    for (int b = 0; b < B && ok; ++b) {
        std::vector<double> prm((size_t)K * 10), y(Q);
        for (size_t i = 0; i < prm.size(); ++i) prm[i] = params[(size_t)b * K * 10 + i];
        for (int i = 0; i < Q; ++i) y[i] = labf[(size_t)b * Q + i];
        const float* qb = &q[(size_t)(shared ? 0 : b) * Q * 3];
        std::vector<double> R((size_t)K * 9);
        for (int k = 0; k < K; ++k) { double M[3][3]; rotation64(&prm[(size_t)k * 10 + 3], M); for (int i = 0; i < 9; ++i) R[(size_t)k * 9 + i] = M[i / 3][i % 3]; }
        for (int i = 0; i < Q; ++i) {
            const Query64 r = query64(prm.data(), R, kinds.data(), K, qb + (size_t)i * 3, y[i], tau);
            want[0] += r.bce; want[1] += r.ov; want_skipped += r.skipped;
            const float gl = lse[(size_t)b * Q + i], gs = s[(size_t)b * Q + i];
            if (std::isfinite(r.l)) worst_q = std::max(worst_q, fabs(gl - r.l) / (1 + fabs(r.l))); else ok = ok && (gl == (float)r.l);
            worst_q = std::max(worst_q, fabs(gs - r.s) / (1 + fabs(r.s)));
        }
        for (int k = 0; k < K; ++k) for (int c = 0; c < 10; ++c) {          // central differences of the double loss
            const size_t at = (size_t)k * 10 + c;
            if (dead[(size_t)b * K + k]) continue;
            const double keep = prm[at], h = 1e-6 * std::max(1.0, fabs(keep));
            prm[at] = keep + h; const double up = sample64(prm.data(), kinds.data(), K, qb, y.data(), Q, tau, g[0], g[1]);
            prm[at] = keep - h; const double dn = sample64(prm.data(), kinds.data(), K, qb, y.data(), Q, tau, g[0], g[1]);
            prm[at] = keep;
            grad[(size_t)b * K * 10 + at] = (up - dn) / (2 * h) / ((double)B * Q);
        }
    }
    for (size_t i = 0; i < grad.size() && ok; ++i) {
        gmax = std::max(gmax, fabs(grad[i]));
        if (!std::isfinite(dp[i])) { ++nonfinite; continue; }
        if (dead[i / 10]) dead_wrong += dp[i] != 0.0f; else worst_g = std::max(worst_g, fabs(dp[i] - grad[i]));
    }
    const double e0 = fabs(out[0] - want[0] / ((double)B * Q)) / (1 + fabs(want[0] / ((double)B * Q))), e1 = fabs(out[1] - want[1] / ((double)B * Q)) / (1 + fabs(want[1] / ((double)B * Q)));
    // central differences carry their own error (a cuboid's maximum changes axis, q3 wraps): 2e-3 of the largest component
    ok = ok && e0 <= 1e-5 && e1 <= 1e-5 && worst_q <= 1e-4 && skipped[0] == want_skipped && nonfinite == 0 && dead_wrong == 0 && worst_g <= 2e-3 * std::max(gmax, 1e-30);
    printf("%-40s B %3d K %3d Q %5d  plan %2d x %4d%s  losses %.1e %.1e  per query %.1e  skipped %4lld  grad %.1e of %.1e  %s\n", name, B, K, Q, slices, slice,
           qpl ? " (direct)" : "", e0, e1, worst_q, want_skipped, worst_g, gmax, ok ? "ok" : "FAILED");
    for (void* p : {(void*)d_p, (void*)d_q, (void*)d_g, (void*)d_k, d_l, ws, ws2, (void*)lse, (void*)s, (void*)lse2, (void*)s2, (void*)out, (void*)dp, (void*)skipped}) free(p);
    return !ok;
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    bad += run("shared queries, uint8 labels", 2, 3, 300, true, true, 0.05f, false, 0);
    bad += run("K = 1, Q = 1", 1, 1, 1, false, false, 0.1f, false, 0);
    bad += run("two stagings, fp32 labels", 1, 300, 40, false, false, 0.1f, false, 0);
    bad += run("three slices + 1", 2, 4, 769, false, true, 0.05f, false, 0);
    bad += run("NaN / inf / zero extent", 3, 5, 270, false, false, 0.05f, true, 0);
    bad += run("NaN / inf / zero extent, shared, uint8", 2, 2, 70, true, true, 0.02f, true, 0);
    bad += run("two queries a lane", 2, 2, 513, false, true, 0.05f, false, 2);
    bad += run("four queries a lane", 1, 3, 1030, true, false, 0.05f, false, 4);
    bad += run("eight queries a lane, hostile", 2, 4, 2049, false, false, 0.05f, true, 8);
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; alignas(16) double st[64]; int32_t i4[4] = {0, 0, 0, 0};
        const int big = VPN_OCCUPANCY_MAX_ITEMS + 1;
        auto fwd = [&](int null_at, int B, int K, int Q, float tau, void* ws, size_t bytes) { const void* p[8] = {v, i4, v, v, v, v, v, i4}; if (null_at >= 0) p[null_at] = nullptr;
            return vpn_occloss_fwd((const float*)p[0], (const int32_t*)p[1], (const float*)p[2], 1, p[3], 0, B, K, Q, tau, ws, bytes, (float*)p[4], (float*)p[5], (float*)p[6], (int32_t*)p[7], nullptr); };
        auto bwd = [&](int null_at, int B, int K, int Q, float tau, void* ws, size_t bytes) { const void* p[8] = {v, v, i4, v, v, v, v, v}; if (null_at >= 0) p[null_at] = nullptr;
            return vpn_occloss_bwd((const float*)p[0], (const float*)p[1], (const int32_t*)p[2], (const float*)p[3], 1, p[4], 0, (const float*)p[5], (const float*)p[6], B, K, Q, tau, ws, bytes, (float*)p[7], nullptr); };
        bool ok = true;
        for (int k : {0, 1, 2, 3, 4, 5, 6}) ok = ok && fwd(k, 1, 1, 1, 0.05f, st, 512) == VPN_E_BADARG;      // out NULL: n_skipped may not be given
        for (int k = 0; k < 8; ++k) ok = ok && bwd(k, 1, 1, 1, 0.05f, st, 512) == VPN_E_BADARG;
        for (float tau : {0.0f, -1.0f, NAN, INFINITY}) ok = ok && fwd(-1, 1, 1, 1, tau, st, 512) == VPN_E_BADARG && bwd(-1, 1, 1, 1, tau, st, 512) == VPN_E_BADARG;
        for (int k = 0; k < 3; ++k) { int a[3] = {1, 1, 1}; a[k] = 0; ok = ok && fwd(-1, a[0], a[1], a[2], 0.05f, st, 512) == VPN_E_BADARG && bwd(-1, a[0], a[1], a[2], 0.05f, st, 512) == VPN_E_BADARG; }
        ok = ok && fwd(-1, 65536, 1, 1, 0.05f, st, 512) == VPN_E_TOOBIG && fwd(-1, 1, VPN_MAX_PRIMS + 1, 1, 0.05f, st, 512) == VPN_E_TOOBIG && fwd(-1, 1, 1, big, 0.05f, st, 512) == VPN_E_TOOBIG;
        ok = ok && bwd(-1, 65536, 1, 1, 0.05f, st, 512) == VPN_E_TOOBIG && bwd(-1, 1, VPN_MAX_PRIMS + 1, 1, 0.05f, st, 512) == VPN_E_TOOBIG && bwd(-1, 1, 1, big, 0.05f, st, 512) == VPN_E_TOOBIG;
        ok = ok && fwd(-1, 1, 1, 1, 0.05f, nullptr, 512) == VPN_E_BADARG && fwd(-1, 1, 1, 1, 0.05f, st, 15) == VPN_E_BADARG && fwd(-1, 1, 1, 1, 0.05f, (char*)st + 8, 504) == VPN_E_BADARG;
        ok = ok && bwd(-1, 1, 1, 1, 0.05f, nullptr, 512) == VPN_E_BADARG && bwd(-1, 1, 1, 1, 0.05f, st, 191) == VPN_E_BADARG && bwd(-1, 1, 1, 1, 0.05f, (char*)st + 8, 504) == VPN_E_BADARG;
        ok = ok && vpn_occloss_workspace(1, 1, 1) == 192 && vpn_occloss_workspace(2, 3, 257) == 2 * 2 * 4 * 3 * 48 && vpn_occloss_workspace(0, 1, 1) == 0 && vpn_occloss_workspace(1, 1, big) == 0 && vpn_occloss_workspace(1, VPN_MAX_PRIMS + 1, 1) == 0;
        int sq = 0;
        ok = ok && vpn_occloss_plan(64, 32768, &sq) == 16 && sq == 2048 && vpn_occloss_plan(2, 257, &sq) == 2 && sq == 256 && vpn_occloss_plan(128, 513, &sq) == 2 && sq == 512;
        ok = ok && vpn_occloss_plan(3, 700, nullptr) == 3 && vpn_occloss_plan(0, 1, &sq) == VPN_E_BADARG && vpn_occloss_plan(1, 0, &sq) == VPN_E_BADARG && vpn_occloss_plan(65536, 1, &sq) == VPN_E_TOOBIG && vpn_occloss_plan(1, big, &sq) == VPN_E_TOOBIG;
        printf("%-99s %s\n", "argument validation, plan and workspace sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf("%.0f s of wall time\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
