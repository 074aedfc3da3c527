// Host check of csrc/fcstack.hip without a GPU: the kernels' own source is compiled as C++ against the shim in
// hip/hip_runtime.h, which runs a launch workgroup by workgroup on std::threads (one per work-item, real barriers,
// __shfl_xor through a per-wave exchange buffer), and vpn_fc_stack_fwd / _bwd are compared with a float64 restatement:
// every layer's activations, the epilogues, dX, dW, db; buffers have their exact sizes, so AddressSanitizer sees any
// access past an end.  It checks indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/fcstack_host/main.cpp -o fc_host
//   ASAN_OPTIONS=detect_leaks=0 ./fc_host          (the check leaks its buffers on purpose: it exits right after)
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64];
#include "../../volumetric-primitives-net_amd/csrc/fcstack.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cstdio>
#include <random>
static std::mt19937 rng(1);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
static float* al(size_t n, bool off) { float* p = (float*)malloc((n + (off ? 1 : 0)) * 4); return off ? p + 1 : p; }
int run(int G, int L, int B, const int* in0, int hidden, const int* outs, int epi, int drop, bool misalign) {
    VpnFcStack s{}; VpnFcGrad gr{}; s.G = G; s.L = L; s.B = B;
    std::vector<std::vector<double>> ref_act(G * L), dyv(G * L);
    std::vector<float*> W(G * L), Bi(G * L), dW(G * L), dB(G * L), X(G), dX(G); std::vector<uint8_t*> M(G * L);
    int K = outs[0] / 3, maxw = 0;
    for (int g = 0; g < G; ++g) {
        s.in0[g] = in0[g]; X[g] = al((size_t)B * in0[g], misalign); dX[g] = al((size_t)B * in0[g], false);
        for (size_t i = 0; i < (size_t)B * in0[g]; ++i) X[g][i] = rnd();
        s.x[g] = X[g]; gr.dx[g] = dX[g]; int w = in0[g]; maxw = std::max(maxw, w);
        for (int l = 0; l < L; ++l) {
            int i = g * L + l, o = l == L - 1 ? outs[g] : hidden; s.out[i] = o; maxw = std::max(maxw, o);
            W[i] = al((size_t)o * w, false); Bi[i] = al(o, false); dW[i] = al((size_t)o * w, false); dB[i] = al(o, false);
            for (size_t e = 0; e < (size_t)o * w; ++e) W[i][e] = rnd() / sqrtf(w);
            for (int e = 0; e < o; ++e) Bi[i][e] = 0.1f * rnd();
            M[i] = (uint8_t*)malloc((size_t)B * o); for (size_t e = 0; e < (size_t)B * o; ++e) M[i][e] = rng() & 1;
            s.w[i] = W[i]; s.bias[i] = Bi[i]; s.keep[i] = M[i]; s.act[i] = al((size_t)B * o, false);
            gr.dw[i] = dW[i]; gr.db[i] = dB[i]; w = o;
        }
    }
    if (G > 1) { gr.dw[0] = nullptr; gr.db[0] = nullptr; }        // a frozen slot
    size_t fin_n = epi == 2 ? (size_t)B * K * 10 : (size_t)B * outs[0];
    float* fin = al(fin_n, false);
    int rc = vpn_fc_stack_fwd(s, drop, 0.5f, 5, nullptr, epi, K, 1, 0.01f, 0.8f, 8, 10, 10, epi ? fin : nullptr, nullptr);
    if (rc) { printf("fwd rc %d\n", rc); return 1; }
    // reference forward in double
    double worst = 0;
    for (int g = 0; g < G; ++g) { int w = in0[g]; std::vector<double> h(X[g], X[g] + (size_t)B * w);
        for (int l = 0; l < L; ++l) { int i = g * L + l, o = s.out[i]; std::vector<double> y((size_t)B * o);
            for (int b = 0; b < B; ++b) for (int r = 0; r < o; ++r) { double a = Bi[i][r]; for (int c = 0; c < w; ++c) a += h[(size_t)b * w + c] * W[i][(size_t)r * w + c];
                if (l < L - 1 && drop == 1) a = M[i][(size_t)b * o + r] ? a * 2 : 0; y[(size_t)b * o + r] = a; }
            double mx = 1e-30, er = 0; for (size_t e = 0; e < y.size(); ++e) { mx = std::max(mx, fabs(y[e])); er = std::max(er, fabs(y[e] - s.act[i][e])); }
            worst = std::max(worst, er / mx); ref_act[i] = y; h = y; w = o; } }
    printf("  fwd act rel err %.2e\n", worst);
    // backward: gout random; reference dY of last layer
    std::vector<float*> go(G); size_t ws = vpn_fc_stack_workspace(G, B, maxw); void* wsp = aligned_alloc(64, (ws + 63) / 64 * 64);
    if (epi == 0) for (int g = 0; g < G; ++g) { go[g] = al((size_t)B * outs[g], false); for (size_t e = 0; e < (size_t)B * outs[g]; ++e) go[g][e] = rnd(); gr.gout[g] = go[g]; }
    else { go[0] = al(fin_n, false); for (size_t e = 0; e < fin_n; ++e) go[0][e] = rnd(); gr.gout[0] = go[0]; }
    rc = vpn_fc_stack_bwd(s, gr, drop, 0.5f, 5, nullptr, epi, K, 1, 0.01f, 0.8f, 8, 10, 10, wsp, ws, nullptr);
    if (rc) { printf("bwd rc %d\n", rc); return 1; }
    worst = 0;
    for (int g = 0; g < G; ++g) {
        int o = outs[g]; std::vector<double> dy((size_t)B * o);
        for (int b = 0; b < B; ++b) for (int r = 0; r < o; ++r) { size_t e = (size_t)b * o + r; double raw = ref_act[g * L + L - 1][e];
            if (epi == 0) dy[e] = go[g][e];
            else if (epi == 1) { double t = tanh(raw); dy[e] = go[0][e] * (1 - t * t); double fe = fabs(t - fin[e]); worst = std::max(worst, fe); }
            else { int wdt = g == 1 ? 4 : 3, f0 = g == 0 ? 0 : (g == 1 ? 3 : 7), k = r / wdt, f = f0 + r % wdt; double y, d;
                if (f < 7) { double sg = 1 / (1 + exp(-raw)); y = f < 3 ? sg + 0.1 : sg; d = sg * (1 - sg); } else { y = tanh(raw); d = 1 - y * y; }
                if (f < 3) { double rr = f == 0 ? 8 : 10; y /= rr; d /= rr; }
                size_t pe = ((size_t)b * K + k) * 10 + f; worst = std::max(worst, fabs(y - fin[pe])); dy[e] = go[0][pe] * d; } }
        for (int l = L - 1; l >= 0; --l) { int i = g * L + l, oo = s.out[i], w = l == 0 ? in0[g] : s.out[i - 1];
            std::vector<double> xin = l == 0 ? std::vector<double>(X[g], X[g] + (size_t)B * w) : ref_act[i - 1];
            double mx = 1e-30, er = 0, mb = 1e-30, eb = 0;
            for (int r = 0; r < oo; ++r) { double sb = 0; for (int b = 0; b < B; ++b) sb += dy[(size_t)b * oo + r];
                if (gr.db[i]) { mb = std::max(mb, fabs(sb)); eb = std::max(eb, fabs(sb - dB[i][r])); }
                if (gr.dw[i]) for (int c = 0; c < w; ++c) { double a = 0; for (int b = 0; b < B; ++b) a += dy[(size_t)b * oo + r] * xin[(size_t)b * w + c];
                    mx = std::max(mx, fabs(a)); er = std::max(er, fabs(a - dW[i][(size_t)r * w + c])); } }
            worst = std::max(worst, std::max(er / mx, eb / mb));
            std::vector<double> dx((size_t)B * w);
            for (int b = 0; b < B; ++b) for (int c = 0; c < w; ++c) { double a = 0; for (int r = 0; r < oo; ++r) a += dy[(size_t)b * oo + r] * W[i][(size_t)r * w + c];
                if (l > 0 && drop == 1) a = M[i - 1][(size_t)b * w + c] ? a * 2 : 0; dx[(size_t)b * w + c] = a; }
            if (l == 0) { double m2 = 1e-30, e2 = 0; for (size_t e = 0; e < dx.size(); ++e) { m2 = std::max(m2, fabs(dx[e])); e2 = std::max(e2, fabs(dx[e] - dX[g][e])); } worst = std::max(worst, e2 / m2); }
            dy = dx; } }
    printf("  bwd + epilogue worst rel err %.2e\n", worst);
    return worst > 1e-4;
}
int main() {
    int bad = 0;
    { int in0[3] = {37, 37, 37}, outs[3] = {15, 20, 15}; puts("odd, B=1, vp_pack"); bad += run(3, 3, 1, in0, 41, outs, 2, 0, false); }
    { int in0[3] = {40, 40, 40}, outs[3] = {15, 20, 15}; puts("vec, B=19, mask dropout, vp_pack"); bad += run(3, 3, 19, in0, 72, outs, 2, 1, false); }
    { int in0[3] = {40, 40, 40}, outs[3] = {15, 20, 15}; puts("misaligned x, B=3, none"); bad += run(3, 2, 3, in0, 72, outs, 0, 0, true); }
    { int in0[1] = {1100}, outs[1] = {70}; puts("G=1, long rows, tanh, B=17"); bad += run(1, 2, 17, in0, 36, outs, 1, 0, false); }
    { int in0[2] = {40, 24}, outs[2] = {9, 6}; puts("L=1, mixed widths, B=70"); bad += run(2, 1, 70, in0, 0, outs, 0, 0, false); }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
