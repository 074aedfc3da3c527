// Host check of csrc/trunknorm.hip without a GPU, in the manner of tools/fcstack_host and tools/optim_host: the kernels' own
// source is compiled as C++ against that shim (a launch runs workgroup by workgroup on std::threads, one per work-item, real
// barriers, __shfl_xor through a per-wave exchange buffer), and vpn_bn_act_fwd / _bwd are compared with a float64
// restatement: y, the saved and running statistics, the counter, dx, d_residual, d_weight, d_bias, training and eval, with
// and without ReLU and residual, with outputs that are not wanted left NULL.  Every buffer has its exact size, so
// AddressSanitizer sees any access past an end: odd H W (element accesses), N below one wave, the 16-byte path, ragged
// slices whose rows cross slice boundaries, both sides of VPN_BN_ONE_PASS_MAX, pointers 4 bytes past a 16-byte boundary.
// It checks indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/trunknorm_host/main.cpp -o tn_host
//   ASAN_OPTIONS=detect_leaks=0 ./tn_host          (the check leaks its buffers on purpose: it exits right after)
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

static int run(int B, int C, int H, int W, int relu, int has_res, int training, bool off, float shift, int skip) {
    const size_t HW = (size_t)H * W, N = HW * B, T = N * C;
    const float eps = 1e-5f, mom = 0.1f;
    float *x = al(T, off), *res = has_res ? al(T, off) : nullptr, *y = al(T, off), *dy = al(T, off);
    float *w = al(C, false), *b = al(C, false), *rm = al(C, false), *rv = al(C, false), *sm = al(C, false), *si = al(C, false);
    long long* nbt = (long long*)malloc(8); *nbt = 4;
    for (size_t i = 0; i < T; ++i) { x[i] = shift + (shift != 0 ? 0.05f : 1.0f) * rnd(); if (res) res[i] = rnd(); dy[i] = rnd(); }
    for (int c = 0; c < C; ++c) { w[c] = 1 + 0.3f * rnd(); b[c] = 0.3f * rnd(); rm[c] = shift + 0.1f * rnd(); rv[c] = (shift != 0 ? 0.0025f : 1.0f) * (1 + 0.2f * fabsf(rnd())); }
    std::vector<double> rm0(rm, rm + C), rv0(rv, rv + C);
    const size_t wsb = vpn_bn_act_workspace(B, C, H, W);
    if ((N > VPN_BN_ONE_PASS_MAX) != (wsb != 0)) { puts("  workspace size and regime disagree"); return 1; }
    void* ws = wsb ? malloc(wsb) : nullptr;
    int rc = vpn_bn_act_fwd(x, res, w, b, rm, rv, nbt, B, C, H, W, training, mom, eps, relu, y, training ? sm : nullptr,
                            training ? si : nullptr, training ? ws : nullptr, training ? wsb : 0, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    // ---- float64 restatement
    std::vector<double> Y(T), mean(C), inv(C), RM(C), RV(C), DX(T), DR(T), DW(C), DB(C), G(T);
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
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) {
            const size_t e = ((size_t)bb * C + c) * HW + i;
            double v = (x[e] - mu) * inv[c] * w[c] + b[c]; if (res) v += res[e];
            Y[e] = relu && v < 0 ? 0 : v;
            G[e] = relu && !(y[e] > 0) ? 0 : dy[e];          // the mask of the saved output, as the kernel reads it
            sg += G[e]; sgx += G[e] * (x[e] - mu) * inv[c];
        }
        DB[c] = sg; DW[c] = sgx;
        for (int bb = 0; bb < B; ++bb) for (size_t i = 0; i < HW; ++i) {
            const size_t e = ((size_t)bb * C + c) * HW + i;
            const double xh = (x[e] - mu) * inv[c];
            DX[e] = training ? w[c] * inv[c] * (G[e] - sg / N - xh * sgx / N) : G[e] * w[c] * inv[c];
            DR[e] = G[e];
        }
    }
    int bad = 0;
    cmp(y, Y);
    if (training) { std::vector<double> I(inv); cmp(sm, mean); cmp(si, I); }
    cmp(rm, RM); cmp(rv, RV);
    if (*nbt != 4 + (training ? 1 : 0)) { puts("  counter"); ++bad; }
    // ---- backward; skip: 0 everything wanted, 1 no affine gradients, 2 no dx
    float *dx = skip == 2 ? nullptr : al(T, off), *dr = has_res && relu ? al(T, off) : nullptr;
    float *dw = skip == 1 ? nullptr : al(C, false), *db = skip == 1 ? nullptr : al(C, false);
    rc = vpn_bn_act_bwd(dy, x, relu ? y : nullptr, w, training ? sm : rm, training ? si : rv, B, C, H, W, training, eps, relu, dx,
                        dr, dw, db, ws, wsb, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    if (dx) cmp(dx, DX);
    if (dr) cmp(dr, DR);
    if (dw) { cmp(dw, DW); cmp(db, DB); }
    return bad;
}

int main(int argc, char** argv) {          // an argument: only the shapes whose description contains it
    struct Shape { int B, C, H, W; bool off; float shift; const char* what; };
    const Shape shapes[] = {
        {2, 3, 5, 7, false, 0, "odd H W: element accesses, one wave"},
        {3, 64, 4, 4, false, 0, "N = 48 below one wave, 16-byte accesses"},
        {2, 8, 64, 64, false, 0, "N = 8192 = the one-launch limit, 16-byte accesses"},
        {2, 8, 64, 64, false, 10, "the same around 10 with sigma 0.05 (cancellation)"},
        {2, 4, 64, 64, true, 0, "the same 4 bytes past a 16-byte boundary: elements"},
        {5, 6, 33, 31, false, 0, "ragged: B = 5, H W = 1023"},
        {2, 3, 64, 65, false, 0, "N = 8320 just above the limit: two launches, 16-byte"},
        {3, 2, 53, 53, false, 0, "N = 8427, odd H W: two launches, elements"},
        {5, 2, 45, 41, true, 0, "N = 9225, rows cross slices, misaligned"},
        {9, 2, 32, 36, false, 0, "N = 10368, H W = 1152: slices cross rows, 16-byte"},
    };
    int bad = 0;
    for (const Shape& s : shapes) {
        if (argc > 1 && !strstr(s.what, argv[1])) continue;
        worst = 0; int b = 0, cases = 0;
        for (int training = 1; training >= 0; --training) for (int relu = 0; relu < 2; ++relu) for (int res = 0; res < 2; ++res) {
            b += run(s.B, s.C, s.H, s.W, relu, res, training, s.off, s.shift, (cases++) % 3);
        }
        const double tol = s.shift != 0 ? 2e-4 : 2e-5;      // fp32 against float64; the mean around 10 carries ulp(10) / sigma
        printf("(%d,%3d,%3d,%3d) %-58s worst rel err %.2e  %s\n", s.B, s.C, s.H, s.W, s.what, worst, b || worst > tol ? "FAILED" : "ok");
        bad += b || worst > tol;
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; long long n = 0;
        const int ok = vpn_bn_act_fwd(nullptr, nullptr, v, v, v, v, &n, 1, 1, 2, 2, 1, 0.1f, 1e-5f, 1, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_act_fwd(v, nullptr, v, v, v, v, &n, 1, 1, 1, 1, 1, 0.1f, 1e-5f, 1, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_act_fwd(v, nullptr, v, v, v, v, &n, 0, 1, 2, 2, 1, 0.1f, 1e-5f, 1, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_act_fwd(v, nullptr, v, v, v, v, &n, 4, 1, 64, 64, 1, 0.1f, 1e-5f, 1, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_act_fwd(v, nullptr, v, v, v, v, &n, 65536, 1, 2048, 1, 1, 0.1f, 1e-5f, 1, v, v, v, v, 16, nullptr) == VPN_E_TOOBIG &&
                       vpn_bn_act_fwd(v, nullptr, v, v, nullptr, v, &n, 1, 1, 2, 2, 0, 0.1f, 1e-5f, 1, v, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_act_bwd(v, v, nullptr, v, v, v, 1, 1, 2, 2, 1, 1e-5f, 1, v, nullptr, v, v, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_bn_act_bwd(v, v, v, v, v, v, 1, 1, 2, 2, 1, 1e-5f, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0 &&
                       vpn_bn_act_workspace(2, 3, 64, 65) == 3 * 5 * 2 * sizeof(float) && vpn_bn_act_workspace(2, 8, 64, 64) == 0 && n == 0;
        printf("%-77s %s\n", "argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
