// Host check of csrc/optim.hip without a GPU, in the manner of tools/fcstack_host: the kernel's own source is compiled as C++
// against that shim (a launch runs workgroup by workgroup on std::threads, one per work-item, real barriers) plus
// hip_atomics.h beside this file, and vpn_adam_step is compared with a float64 restatement of Adam.  Every buffer has its
// exact size, so AddressSanitizer sees any access past an end: odd sizes, a misaligned segment, segments that cross a chunk
// boundary, an empty segment, zero segments, and the last-arriver advance of the state over three consecutive launches.
// It checks indexing, the tables and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -ffp-contract=off -fsanitize=address -Itools/fcstack_host -Itools/optim_host \
//       -x c++ tools/optim_host/main.cpp -o optim_host
//   ASAN_OPTIONS=detect_leaks=0 ./optim_host       (the check leaks its buffers on purpose: it exits right after)
#include "hip/hip_runtime.h"
#include "hip_atomics.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64];
#include "../../volumetric-primitives-net_amd/csrc/optim.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cstdio>
#include <random>
static std::mt19937 rng(1);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
// n floats that end where their allocation ends; `off`: begin 4 bytes past a 16-byte boundary
static float* al(size_t n, bool off) { float* p = (float*)malloc((n + (off ? 1 : 0)) * 4 + (n == 0 && !off)); return off ? p + 1 : p; }
struct State { long long step; double b1pow, b2pow; unsigned arrivals, pad; };

int run(const char* what, const std::vector<long long>& sizes, int misaligned, double wd, int zero, bool use_lr_dev) {
    const int S = (int)sizes.size(), CH = VPN_ADAM_CHUNK;
    const double beta1 = 0.9, beta2 = 0.99, eps = 1e-8, lr = 1e-3;
    std::vector<VpnAdamSegment> seg(S); std::vector<long long> chunks;
    std::vector<std::vector<double>> P(S), M(S), V(S);
    for (int s = 0; s < S; ++s) {
        const long long n = sizes[s]; const bool off = s == misaligned;
        seg[s] = VpnAdamSegment{al(n, off), al(n, false), al(n, false), al(n, false), n, off ? 0 : 1};
        for (long long i = 0; i < n; ++i) { seg[s].p[i] = rnd(); seg[s].g[i] = 0.1f * rnd(); seg[s].m[i] = 0.f; seg[s].v[i] = 0.f; }
        P[s].assign(seg[s].p, seg[s].p + n); M[s].assign(n, 0.0); V[s].assign(n, 0.0);
        for (long long f = 0; f < n; f += CH) { chunks.push_back(s); chunks.push_back(f); }
    }
    const int C = (int)chunks.size() / 2;
    // exact-size copies of the tables, as the device would hold them
    VpnAdamSegment* dseg = (VpnAdamSegment*)malloc(sizeof(VpnAdamSegment) * (S ? S : 1)); memcpy(dseg, seg.data(), sizeof(VpnAdamSegment) * S);
    long long* dch = (long long*)malloc(16 * (C ? C : 1)); memcpy(dch, chunks.data(), 16 * (size_t)C);
    State* st = (State*)malloc(sizeof(State)); *st = State{0, 1.0, 1.0, 0u, 0u};
    float* lr_dev = (float*)malloc(4);
    double hyper[5] = {lr, beta1, beta2, eps, wd}, b1 = 1.0, b2 = 1.0, worst = 0;
    int bad = 0;
    for (int step = 1; step <= 3; ++step) {
        const double lr_now = use_lr_dev ? (double)(*lr_dev = 1e-3f * step) : lr;
        std::vector<std::vector<float>> G(S);
        for (int s = 0; s < S; ++s) { for (long long i = 0; i < sizes[s]; ++i) seg[s].g[i] = 0.1f * rnd(); G[s].assign(seg[s].g, seg[s].g + sizes[s]); }
        const int rc = vpn_adam_step(dseg, S, dch, C, st, hyper, use_lr_dev ? lr_dev : nullptr, zero, nullptr);
        if (rc) { printf("  rc %d\n", rc); return 1; }
        b1 *= beta1; b2 *= beta2;
        if (S == 0) { b1 = b2 = 1.0; if (st->step != 0 || st->b1pow != 1.0 || st->b2pow != 1.0 || st->arrivals) { puts("  zero segments advanced the state"); ++bad; } continue; }
        if (st->step != step || st->b1pow != b1 || st->b2pow != b2 || st->arrivals != 0) { printf("  state after launch %d: step %lld arrivals %u\n", step, st->step, st->arrivals); ++bad; }
        for (int s = 0; s < S; ++s) for (long long i = 0; i < sizes[s]; ++i) {
            const double g1 = wd != 0 ? G[s][i] + wd * P[s][i] : G[s][i];
            M[s][i] += (1 - beta1) * (g1 - M[s][i]); V[s][i] = V[s][i] * beta2 + (1 - beta2) * g1 * g1;
            P[s][i] -= lr_now / (1 - b1) * M[s][i] / (sqrt(V[s][i]) / sqrt(1 - b2) + eps);
            worst = std::max(worst, fabs(P[s][i] - seg[s].p[i]) / (fabs(P[s][i]) + 1e-3));
            worst = std::max(worst, fabs(M[s][i] - seg[s].m[i]) / (fabs(M[s][i]) + 1e-3));
            worst = std::max(worst, fabs(V[s][i] - seg[s].v[i]) / (fabs(V[s][i]) + 1e-3));
            if (zero ? seg[s].g[i] != 0.f : seg[s].g[i] != G[s][i]) ++bad;
        }
    }
    printf("%-58s chunks %2d  worst rel err %.2e  %s\n", what, C, worst, bad || worst > 1e-5 ? "FAILED" : "ok");
    return bad || worst > 1e-5;
}
int main() {
    const long long CH = VPN_ADAM_CHUNK;
    int bad = 0;
    bad += run("odd sizes 1 3 4 5 7 255 257, no decay", {1, 3, 4, 5, 7, 255, 257}, -1, 0.0, 0, false);
    bad += run("chunk edges CHUNK-1 CHUNK CHUNK+1 2CHUNK+7 0, decay, zeroing", {CH - 1, CH, CH + 1, 2 * CH + 7, 0}, -1, 1e-6, 1, false);
    bad += run("misaligned p (elements only) beside aligned ones", {CH + 5, 2 * CH + 3, 9}, 1, 1e-6, 1, false);
    bad += run("device learning rate, changed between launches", {CH + 1, 130}, -1, 0.0, 0, true);
    bad += run("zero segments", {}, -1, 0.0, 1, false);
    {   // validation without a launch
        double hyper[5] = {1e-3, 0.9, 0.99, 1e-8, 0}; long long ch[2] = {0, 0}; State st{0, 1.0, 1.0, 0u, 0u}; VpnAdamSegment sg{};
        const int ok = vpn_adam_step(nullptr, 1, ch, 1, &st, hyper, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_adam_step(&sg, 1, ch, 0, &st, hyper, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_adam_step(&sg, 1, ch, -3, &st, hyper, nullptr, 0, nullptr) == VPN_E_BADARG &&
                       vpn_adam_step(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) == 0 &&
                       vpn_adam_table_bytes(3, 2 * CH + 7) == 3 * 48 + 16 * (2 + 3);
        printf("%-58s %s\n", "argument validation and table size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
