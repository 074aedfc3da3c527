// Host check of the stem's pool kernels (the tp_ kernels of csrc/trunknorm.hip) without a GPU, in the manner
// of tools/trunknorm_host: the kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers), and vpn_bn_pool_fwd / _bwd are compared with a
// float64 restatement: p, idx, the saved and running statistics, the counter, dx, d_weight, d_bias, training and eval, with
// outputs that are not wanted left NULL in turn.  Every buffer has its exact size, so AddressSanitizer sees any access past
// an end: windows cut at every border, odd H W, PH = 1, N below one wave, the 16-byte path, both sides of
// VPN_BN_ONE_PASS_MAX, batch rows crossing slices, pointers 4 bytes past a 16-byte boundary.  idx is held to the float64
// windows up to rounding (the named tap lies inside the map and its float64 value within 1e-5 of the float64 maximum); the
// backward is routed by the forward's own idx and p, as the kernel reads them.  It checks indexing, barriers and the
// host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/trunkpool_host/main.cpp -o tp_host
//   ASAN_OPTIONS=detect_leaks=0 ./tp_host          (the check leaks its buffers on purpose: it exits right after)
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64];
// the double form of the shim's __shfl_xor (the merge of the slices sums in double)
static double g_xchd[16][64];
inline double __shfl_xor(double v, int o, int) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xchd[w][l] = v; g_wave[w].wait(); double r = g_xchd[w][l ^ o]; g_wave[w].wait(); return r;
}
#include "../../volumetric-primitives-net_amd/csrc/trunknorm.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cstdio>
#include <random>
static std::mt19937 rng(1);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
// n floats that end where their allocation ends; `off`: begin 4 bytes past a 16-byte boundary
static float* al(size_t n, bool off) { float* p = (float*)malloc((n + (off ? 1 : 0)) * 4); return off ? p + 1 : p; }
static double worst;
static void cmp(const float* got, const std::vector<double>& want) {
    double m = 1e-30, d = 0;
    for (size_t i = 0; i < want.size(); ++i) { m = std::max(m, fabs(want[i])); d = std::max(d, fabs(want[i] - (double)got[i])); }
    worst = std::max(worst, d / m);
}

// skip: 0 everything wanted, 1 no affine gradients, 2 no dx, 3 d_bias alone
static int run(int B, int C, int H, int W, int training, bool off, int skip) {
    const int PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1;
    const size_t HW = (size_t)H * W, N = HW * B, T = N * C, PHW = (size_t)PH * PW, TP = PHW * B * C;
    const float eps = 1e-5f, mom = 0.1f;
    float *x = al(T, off), *p = al(TP, off), *dp = al(TP, off);
    unsigned char* idx = (unsigned char*)malloc(TP);
    float *w = al(C, false), *b = al(C, false), *rm = al(C, false), *rv = al(C, false), *sm = al(C, false), *si = al(C, false);
    long long* nbt = (long long*)malloc(8); *nbt = 4;
    for (size_t i = 0; i < T; ++i) x[i] = rnd();
    for (size_t i = 0; i < TP; ++i) dp[i] = rnd();
    for (int c = 0; c < C; ++c) { w[c] = 1 + 0.3f * rnd(); b[c] = 0.3f * rnd(); rm[c] = 0.1f * rnd(); rv[c] = 1 + 0.2f * fabsf(rnd()); }
    std::vector<double> rm0(rm, rm + C), rv0(rv, rv + C);
    const size_t wsb = vpn_bn_pool_workspace(B, C, H, W);
    if (wsb != (size_t)C * ((N + VPN_BN_SLICE - 1) / VPN_BN_SLICE) * 8) { puts("  workspace size"); return 1; }
    void* ws = malloc(wsb);
    const bool fwd_ws = training && N > VPN_BN_ONE_PASS_MAX;
    int rc = vpn_bn_pool_fwd(x, w, b, rm, rv, nbt, B, C, H, W, training, mom, eps, p, idx, training ? sm : nullptr,
                             training ? si : nullptr, fwd_ws ? ws : nullptr, fwd_ws ? wsb : 0, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    // ---- float64 restatement
    int bad = 0;
    std::vector<double> P(TP), mean(C), inv(C), RM(C), RV(C), DX(T), DW(C), DB(C), G(T, 0.0);
    for (int c = 0; c < C; ++c) {
        double s = 0, m2 = 0;
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) s += x[((size_t)bb * C + c) * HW + i];
        double mu = s / N;
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) { double d = x[((size_t)bb * C + c) * HW + i] - mu; m2 += d * d; }
        double var = m2 / N;
        RM[c] = training ? (1 - (double)mom) * rm0[c] + (double)mom * mu : rm0[c];
        RV[c] = training ? (1 - (double)mom) * rv0[c] + (double)mom * var * N / (N - 1.0) : rv0[c];
        if (!training) { mu = rm0[c]; var = rv0[c]; }
        mean[c] = mu; inv[c] = 1 / sqrt(var + (double)eps);
        for (int bb = 0; bb < B; ++bb) for (int ph = 0; ph < PH; ++ph) for (int pw = 0; pw < PW; ++pw) {
            const size_t m = ((size_t)bb * C + c) * HW, o = ((size_t)bb * C + c) * PHW + (size_t)ph * PW + pw;
            double best = -1;
            for (int r = 0; r < 3; ++r) for (int t = 0; t < 3; ++t) {
                const int h = 2 * ph - 1 + r, ww = 2 * pw - 1 + t;
                if (h < 0 || h >= H || ww < 0 || ww >= W) continue;
                best = std::max(best, std::max((x[m + (size_t)h * W + ww] - mu) * inv[c] * w[c] + b[c], 0.0));
            }
            P[o] = best;
            // the kernel's winner: a tap of the window inside the map that holds the maximum up to rounding
            const int k = idx[o], h = 2 * ph - 1 + k / 3, ww = 2 * pw - 1 + k % 3;
            if (k > 8 || h < 0 || h >= H || ww < 0 || ww >= W) { if (!bad) puts("  idx names a tap outside the map"); ++bad; continue; }
            const double yk = std::max((x[m + (size_t)h * W + ww] - mu) * inv[c] * w[c] + b[c], 0.0);
            if (fabs(yk - best) > 1e-5 * std::max(1.0, best)) { if (!bad) puts("  idx names a tap that is not the maximum"); ++bad; }
            if (p[o] > 0) G[m + (size_t)h * W + ww] += dp[o];         // routed by the forward's own idx and p
        }
        double sg = 0, sgx = 0;
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) {
            const size_t e = ((size_t)bb * C + c) * HW + i;
            sg += G[e]; sgx += G[e] * (x[e] - mu) * inv[c];
        }
        DB[c] = sg; DW[c] = sgx;
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) {
            const size_t e = ((size_t)bb * C + c) * HW + i;
            const double xh = (x[e] - mu) * inv[c];
            DX[e] = training ? w[c] * inv[c] * (G[e] - sg / N - xh * sgx / N) : G[e] * w[c] * inv[c];
        }
    }
    cmp(p, P);
    if (training) { std::vector<double> I(inv); cmp(sm, mean); cmp(si, I); }
    cmp(rm, RM); cmp(rv, RV);
    if (*nbt != 4 + (training ? 1 : 0)) { puts("  counter"); ++bad; }
    // ---- backward
    float *dx = skip == 2 || skip == 3 ? nullptr : al(T, off);
    float *dw = skip == 1 || skip == 3 ? nullptr : al(C, false), *db = skip == 1 ? nullptr : al(C, false);
    const bool bwd_ws = training || dw || db;
    rc = vpn_bn_pool_bwd(dp, x, p, idx, w, training ? sm : rm, training ? si : rv, B, C, H, W, training, eps, dx, dw, db,
                         bwd_ws ? ws : nullptr, bwd_ws ? wsb : 0, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    if (dx) cmp(dx, DX);
    if (dw) cmp(dw, DW);
    if (db) cmp(db, DB);
    return bad;
}

int main(int argc, char** argv) {          // an argument: only the shapes whose description contains it
    struct Shape { int B, C, H, W; bool off; const char* what; };
    const Shape shapes[] = {
        {2, 3, 5, 7, false, "odd H W: element accesses, windows cut at both borders"},
        {3, 64, 4, 4, false, "N = 48 below one wave"},
        {2, 4, 8, 8, false, "16-byte accesses, one wave"},
        {2, 4, 8, 8, true, "the same 4 bytes past a 16-byte boundary: elements"},
        {2, 5, 16, 16, false, "N = 512: the largest slab one wave owns"},
        {1, 4, 19, 27, false, "N = 513: the smallest a whole workgroup owns"},
        {2, 2, 64, 64, false, "N = 8192 = the one-launch limit, 16-byte accesses"},
        {1, 3, 90, 91, false, "N = 8190 just below the limit, odd W"},
        {2, 3, 64, 65, false, "N = 8320 just above: two launches, short last slice"},
        {3, 2, 53, 53, false, "N = 8427, odd H W: two launches, elements"},
        {3, 2, 40, 40, false, "N = 4800: batch rows cross slices, windows straddle them"},
        {3, 2, 60, 52, true, "N = 9360, two launches, W % 4 == 0 but misaligned"},
        {5, 2, 44, 48, false, "N = 10560, two launches, 16-byte accesses, rows cross slices"},
        {2, 64, 32, 32, false, "the stem's channel count"},
        {2, 2, 2, 3, false, "PH = 1"},
        {3, 2, 1, 5, false, "H = 1: one pooled row of windows one row high"},
    };
    int bad = 0;
    for (const Shape& s : shapes) {
        if (argc > 1 && !strstr(s.what, argv[1])) continue;
        worst = 0; int b = 0, cases = 0;
        for (int training = 1; training >= 0; --training) for (int skip = 0; skip < 4; ++skip, ++cases)
            b += run(s.B, s.C, s.H, s.W, training, s.off, skip);
        const double tol = 2e-5;           // fp32 against float64
        printf("(%d,%3d,%3d,%3d) %-62s worst rel err %.2e  %s\n", s.B, s.C, s.H, s.W, s.what, worst, b || worst > tol ? "FAILED" : "ok");
        bad += b || worst > tol;
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; long long n = 0; unsigned char k[4] = {0, 0, 0, 0};
        const int ok = vpn_bn_pool_fwd(nullptr, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, 1e-5f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, 1e-5f, v, nullptr, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 1, 1, 1, 1, 1, 0.1f, 1e-5f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 0, 1, 2, 2, 1, 0.1f, 1e-5f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 1, 1, 2, 2, 1, 1.5f, 1e-5f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, -1.0f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 4, 1, 64, 64, 1, 0.1f, 1e-5f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 4, 1, 64, 64, 1, 0.1f, 1e-5f, v, k, v, v, v, 8, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 65536, 1, 2048, 1, 1, 0.1f, 1e-5f, v, k, v, v, v, 16, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_pool_fwd(v, v, v, v, v, &n, 65535 * 512 + 1, 1, 1, 1, 0, 0.1f, 1e-5f, v, k, v, v, v, 16, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_pool_fwd(v, v, v, nullptr, v, &n, 1, 1, 2, 2, 0, 0.1f, 1e-5f, v, k, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_bwd(v, v, v, nullptr, v, v, v, 1, 1, 2, 2, 1, 1e-5f, v, v, v, v, 16, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_bwd(v, v, v, k, v, v, v, 1, 1, 2, 2, 1, 1e-5f, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_bwd(v, v, v, k, v, v, v, 1, 1, 1, 1, 1, 1e-5f, v, v, v, v, 16, nullptr) == VPN_E_BADARG &&
                       vpn_bn_pool_bwd(v, v, v, k, v, v, v, 1, 1, 2, 2, 1, 1e-5f, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0 &&
                       vpn_bn_pool_workspace(2, 3, 64, 65) == 3 * 5 * 2 * sizeof(float) && vpn_bn_pool_workspace(2, 8, 64, 64) == 8 * 4 * 2 * sizeof(float) &&
                       vpn_bn_pool_workspace(0, 1, 2, 2) == 0 && n == 0;
        printf("%-81s %s\n", "argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
