// Host check of the trunk's tail (the tt_ kernels of csrc/trunknorm.hip) without a GPU, in the manner of
// tools/trunkpool_host: the kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers), and vpn_bn_tail_fwd / _bwd are compared with a
// float64 restatement: y, m, the saved and running statistics, the counter, dx, d_residual, d_weight, d_bias, training and
// eval, every (ReLU, residual) pair, and with ReLU and residual on dy, dm and each output left NULL in turn.  Every buffer
// has its exact size, so AddressSanitizer sees any access past an end.  The shapes are those of tests/test_trunktail.py: the
// real site (all 512 channels for one training step, 16 of them for every case: a work-item is a thread here), N below a wave, odd sizes, both sides of the one-wave and the one-launch limit, rows longer than a slice,
// rows straddling slice ends, HW = 1; two of them again 4 bytes past a 16-byte boundary.  The backward's mask is the
// forward's own y, as the kernel reads it.  It checks indexing, barriers and the host-side launch logic; it says nothing
// about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/trunktail_host/main.cpp -o tt_host
//   ASAN_OPTIONS=detect_leaks=0 ./tt_host          (the check leaks its buffers on purpose: it exits right after)
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

// null: 0 (and 7: without the comparison with vpn_bn_act_fwd) everything given and wanted, 1 dy NULL, 2 dm NULL, 3 no dx, 4 no d_residual, 5 no d_weight, 6 no d_bias
static int run(int B, int C, int H, int W, int training, int relu, int residual, bool off, int null) {
    const size_t HW = (size_t)H * W, N = HW * B, T = N * C, BC = (size_t)B * C;
    const float eps = 1e-5f, mom = 0.1f;
    float *x = al(T, off), *res = residual ? al(T, off) : nullptr, *y = al(T, off), *m = al(BC, false);
    float *dy = null == 1 ? nullptr : al(T, off), *dm = null == 2 ? nullptr : al(BC, false);
    float *w = al(C, false), *b = al(C, false), *rm = al(C, false), *rv = al(C, false), *sm = al(C, false), *si = al(C, false);
    long long* nbt = (long long*)malloc(8); *nbt = 4;
    for (size_t i = 0; i < T; ++i) { x[i] = rnd(); if (res) res[i] = rnd(); if (dy) dy[i] = rnd(); }
    for (size_t i = 0; i < BC; ++i) if (dm) dm[i] = rnd();
    for (int c = 0; c < C; ++c) { w[c] = 1 + 0.3f * rnd(); b[c] = 0.3f * rnd(); rm[c] = 0.1f * rnd(); rv[c] = 1 + 0.2f * fabsf(rnd()); }
    std::vector<double> rm0(rm, rm + C), rv0(rv, rv + C);
    const size_t wsb = vpn_bn_tail_workspace(B, C, H, W);
    if (wsb != (N > VPN_BN_ONE_PASS_MAX ? (size_t)C * ((N + VPN_BN_SLICE - 1) / VPN_BN_SLICE) * 8 : 0) || wsb != vpn_bn_act_workspace(B, C, H, W)) {
        puts("  workspace size"); return 1;
    }
    void* ws = wsb ? malloc(wsb) : nullptr;
    int rc = vpn_bn_tail_fwd(x, res, w, b, rm, rv, nbt, B, C, H, W, training, mom, eps, relu, y, m, training ? sm : nullptr,
                             training ? si : nullptr, training ? ws : nullptr, training ? wsb : 0, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    // ---- float64 restatement
    int bad = 0;
    std::vector<double> Y(T), M(BC), mean(C), inv(C), RM(C), RV(C), DX(T), DR(T), DW(C), DB(C);
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
        double sg = 0, sgx = 0;
        for (int bb = 0; bb < B; ++bb) {
            double row = 0;
            for (size_t i = 0; i < HW; ++i) {
                const size_t e = ((size_t)bb * C + c) * HW + i;
                double v = (x[e] - mu) * inv[c] * w[c] + b[c] + (res ? (double)res[e] : 0.0);
                Y[e] = relu ? std::max(v, 0.0) : v;
                row += Y[e];
                double g = (dy ? (double)dy[e] : 0.0) + (dm ? (double)dm[(size_t)bb * C + c] / (double)HW : 0.0);
                if (relu && !(y[e] > 0)) g = 0;                           // the mask of the forward's own y
                DR[e] = g; sg += g; sgx += g * (x[e] - mu) * inv[c];
            }
            M[(size_t)bb * C + c] = row / (double)HW;
        }
        DB[c] = sg; DW[c] = sgx;
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) {
            const size_t e = ((size_t)bb * C + c) * HW + i;
            const double xh = (x[e] - mu) * inv[c];
            DX[e] = training ? w[c] * inv[c] * (DR[e] - sg / N - xh * sgx / N) : DR[e] * w[c] * inv[c];
        }
    }
    cmp(y, Y); cmp(m, M);
    if (training) { std::vector<double> I(inv); cmp(sm, mean); cmp(si, I); }
    cmp(rm, RM); cmp(rv, RV);
    if (*nbt != 4 + (training ? 1 : 0)) { puts("  counter"); ++bad; }
    // ---- backward
    float *dx = null == 3 ? nullptr : al(T, off), *dres = null == 4 || !residual ? nullptr : al(T, off);
    float *dw = null == 5 ? nullptr : al(C, false), *db = null == 6 ? nullptr : al(C, false);
    rc = vpn_bn_tail_bwd(dy, dm, x, relu ? y : nullptr, w, training ? sm : rm, training ? si : rv, B, C, H, W, training, eps, relu, dx,
                         dres, dw, db, ws, wsb, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    if (dx) cmp(dx, DX);
    if (dres) cmp(dres, DR);
    if (dw) cmp(dw, DW);
    if (db) cmp(db, DB);
    if (null == 2) {                           // dm NULL: vpn_bn_act_bwd bit for bit
        float *dx2 = al(T, off), *dr2 = residual ? al(T, off) : nullptr, *dw2 = al(C, false), *db2 = al(C, false);
        rc = vpn_bn_act_bwd(dy, x, relu ? y : nullptr, w, training ? sm : rm, training ? si : rv, B, C, H, W, training, eps, relu, dx2, dr2,
                            dw2, db2, ws, wsb, nullptr);
        if (rc || memcmp(dx, dx2, T * 4) || (dr2 && memcmp(dres, dr2, T * 4)) || memcmp(dw, dw2, C * 4) || memcmp(db, db2, C * 4)) {
            puts("  dm NULL differs from vpn_bn_act_bwd"); ++bad;
        }
    }
    if (null == 0) {                           // the forward's statistics: vpn_bn_act_fwd bit for bit (y: up to the host compiler's contraction)
        float *y2 = al(T, off), *sm2 = al(C, false), *si2 = al(C, false), *rm2 = al(C, false), *rv2 = al(C, false);
        for (int c = 0; c < C; ++c) { rm2[c] = (float)rm0[c]; rv2[c] = (float)rv0[c]; }
        long long n2 = 4;
        rc = vpn_bn_act_fwd(x, res, w, b, rm2, rv2, &n2, B, C, H, W, training, mom, eps, relu, y2, training ? sm2 : nullptr,
                            training ? si2 : nullptr, training ? ws : nullptr, training ? wsb : 0, nullptr);
        { std::vector<double> Y2(y2, y2 + T); cmp(y, Y2); }
        if (rc || memcmp(rm, rm2, C * 4) || memcmp(rv, rv2, C * 4) || n2 != *nbt ||
            (training && (memcmp(sm, sm2, C * 4) || memcmp(si, si2, C * 4)))) {
            puts("  the forward differs from vpn_bn_act_fwd"); ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv) {          // an argument: only the shapes whose description contains it
    struct Shape { int B, C, H, W; bool off; const char* what; };
    const Shape shapes[] = {
        {8, 512, 4, 4, false, "the real site, once"},
        {8, 16, 4, 4, false, "the real site, 16 of its channels, every case"},
        {3, 64, 4, 4, false, "N = 48 below one wave"},
        {2, 3, 5, 7, false, "odd sizes: element accesses"},
        {2, 5, 16, 16, false, "N = 512: the largest slab one wave owns"},
        {2, 5, 16, 16, true, "the same 4 bytes past a 16-byte boundary: elements"},
        {1, 4, 19, 27, false, "N = 513, B = 1"},
        {2, 8, 64, 64, false, "N = 8192 = the one-launch limit, rows of 4096"},
        {5, 6, 33, 31, false, "ragged"},
        {1, 3, 90, 91, false, "N = 8190 just below the limit"},
        {2, 3, 64, 65, false, "two launches, 16-byte accesses, rows longer than a slice"},
        {2, 3, 64, 65, true, "the same misaligned: elements"},
        {3, 2, 53, 53, false, "two launches, odd rows longer than a slice"},
        {40, 2, 15, 15, false, "two launches, nine rows per workgroup, rows straddle slice ends"},
        {4, 3, 1, 1, false, "HW = 1"},
    };
    int bad = 0;
    for (const Shape& s : shapes) {
        if (argc > 1 && !strstr(s.what, argv[1])) continue;
        worst = 0; int b = 0;
        for (int training = 1; training >= 0; --training) {
            if (s.C == 512) {                  // 32768 threads a launch: the training step with everything wanted alone
                if (training) b += run(s.B, s.C, s.H, s.W, 1, 1, 1, s.off, 7);
                continue;
            }
            for (int pair = 0; pair < 4; ++pair) b += run(s.B, s.C, s.H, s.W, training, pair & 1, pair >> 1, s.off, 0);
            for (int null = 1; null <= 6; ++null) b += run(s.B, s.C, s.H, s.W, training, 1, 1, s.off, null);
        }
        const double tol = 2e-5;           // fp32 against float64
        printf("(%2d,%3d,%3d,%3d) %-66s worst rel err %.2e  %s\n", s.B, s.C, s.H, s.W, s.what, worst, b || worst > tol ? "FAILED" : "ok");
        bad += b || worst > tol;
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; long long n = 0;
        const int ok = vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, 1e-5f, 1, v, nullptr, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 1, 1, 2, 2, 0, 0.1f, 1e-5f, 1, v, nullptr, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(nullptr, v, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, 1e-5f, 1, nullptr, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 1, 1, 1, 1, 1, 0.1f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 0, 1, 2, 2, 1, 0.1f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 1, 1, 2, 2, 1, 1.5f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, -1.0f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, nullptr, v, &n, 1, 1, 2, 2, 0, 0.1f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 4, 1, 64, 64, 1, 0.1f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 4, 1, 64, 64, 1, 0.1f, 1e-5f, 1, v, v, v, v, v, 8, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 65536, 1, 1025, 1, 1, 0.1f, 1e-5f, 1, v, v, v, v, v, 16, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 65536, 1, 1025, 1, 0, 0.1f, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_tail_fwd(v, v, v, v, v, v, &n, 65536, 1, 2048, 1, 1, 0.1f, 1e-5f, 1, v, v, v, v, v, 16, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_tail_bwd(nullptr, nullptr, v, v, v, v, v, 1, 1, 2, 2, 1, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_bwd(v, v, nullptr, v, v, v, v, 1, 1, 2, 2, 1, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_bwd(v, v, v, nullptr, v, v, v, 1, 1, 2, 2, 1, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_bwd(v, v, v, v, v, v, v, 1, 1, 1, 1, 1, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_bwd(v, v, v, v, v, v, v, 4, 1, 64, 64, 1, 1e-5f, 1, v, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_tail_bwd(v, v, v, v, v, v, v, 65536, 1, 1025, 1, 1, 1e-5f, 1, v, v, v, v, v, 16, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_tail_bwd(v, v, v, v, v, v, v, 1, 1, 2, 2, 1, 1e-5f, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0 &&
                       vpn_bn_tail_bwd(nullptr, v, v, v, v, v, v, 4, 1, 64, 64, 1, 1e-5f, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0 &&
                       vpn_bn_tail_workspace(2, 3, 64, 65) == 3 * 5 * 2 * sizeof(float) && vpn_bn_tail_workspace(2, 8, 64, 64) == 0 &&
                       vpn_bn_tail_workspace(0, 1, 2, 2) == 0 && vpn_bn_tail_workspace(65536, 1, 1025, 1) == 0 && n == 0;
        printf("%-85s %s\n", "argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
