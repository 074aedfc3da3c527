// Host check of csrc/trunkfold.hip (and what it takes from csrc/vpn_conv_stride.h and csrc/vpn_conv_gemm.h) without a GPU, in
// the manner of tools/trunkconv_host: the kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a
// launch runs workgroup by workgroup on std::threads, one per work-item, real barriers, the f32-input MFMA emulated with the
// instruction's lane maps and its k-ordered fmaf chain), and vpn_conv2d_bias_act_fwd is compared with one float64 loop.  The
// inputs are small integers, so every product, partial sum and epilogue step is exact in fp32 and the results must EQUAL the
// float64 ones.  Every buffer has its exact size, so AddressSanitizer sees any access past an end; y is filled with NaN before
// the call, so an element the kernels forgot to write is caught.  Every shape runs in the eight combinations of bias,
// residual and ReLU (the large ones in two), and the call without any of the three must equal vpn_conv2d_fwd bit for bit.
// Shapes: every R, the split and the unsplit regime of every R, tails in M, N and K, one chunk, stride 3, padding wider than
// the image, an element count that is a multiple of 4 with 9 pixels a channel (a float4 of the merge holds two channels),
// pointers 4 bytes past a 16-byte boundary (the merge's element path).
// It checks indexing, masking, the epilogue's order and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/trunkfold_host/main.cpp -o tf_host
//   ASAN_OPTIONS=detect_leaks=0 ./tf_host          (the check leaks its buffers on purpose: it exits right after)
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
#include "../../volumetric-primitives-net_amd/csrc/trunkstride.hip"
#include "../../volumetric-primitives-net_amd/csrc/trunkfold.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cmath>
#include <cstdio>
#include <random>
static std::mt19937 rng(1);
static float ri(int a) { return (float)std::uniform_int_distribution<int>(-a, a)(rng); }
// n floats that end where their allocation ends, filled with NaN; `off`: begin 4 bytes past a 16-byte boundary
static float* al(size_t n, bool off) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, (n + (off ? 1 : 0)) * 4)) { puts("no memory"); exit(1); }
    float* p = (float*)q + (off ? 1 : 0);
    for (size_t i = 0; i < n; ++i) p[i] = NAN;
    return p;
}

static int regimes[8][2];          // [R][split]: calls seen
static int vec_straddle;           // split calls on the 16-byte path whose float4s hold two channels

struct Shape { int B, Ci, Co, H, W, R, st, p; bool off; const char* what; };

static int run(const Shape& q, int combo) {
    const int B = q.B, Ci = q.Ci, Co = q.Co, H = q.H, W = q.W, R = q.R, st = q.st, p = q.p;
    const bool use_bias = combo & 1, use_res = combo & 2, relu = combo & 4;
    const int OH = (H + 2 * p - R) / st + 1, OW = (W + 2 * p - R) / st + 1;
    const size_t nx = (size_t)B * Ci * H * W, ny = (size_t)B * Co * OH * OW, nw = (size_t)Co * Ci * R * R;
    float *x = al(nx, q.off), *w = al(nw, q.off), *y = al(ny, q.off), *bias = al(Co, q.off), *res = al(ny, q.off);
    for (size_t i = 0; i < nx; ++i) x[i] = ri(3);
    for (size_t i = 0; i < nw; ++i) w[i] = ri(2);
    for (int i = 0; i < Co; ++i) bias[i] = ri(9);
    for (size_t i = 0; i < ny; ++i) res[i] = ri(9);
    const int S = vpn_conv2d_splits(B, Ci, Co, H, W, R, st, p, VPN_CONV_FWD);
    if (S < 1) { printf("  splits %d\n", S); return 1; }
    ++regimes[R][S > 1];
    const size_t wf = vpn_conv2d_workspace(B, Ci, Co, H, W, R, st, p, VPN_CONV_FWD);
    if (wf != (S > 1 ? S * ny * 4 : 0)) { puts("  workspace size and regime disagree"); return 1; }
    if (S > 1 && !q.off && ny % 4 == 0 && (OH * OW) % 4 != 0) ++vec_straddle;
    void* ws = nullptr;                                  // 16-byte aligned, exact size
    if (wf && posix_memalign(&ws, 16, wf)) { puts("  no memory"); return 1; }
    int rc = vpn_conv2d_bias_act_fwd(x, w, use_bias ? bias : nullptr, use_res ? res : nullptr, y, B, Ci, Co, H, W, R, st, p, relu, ws, wf, nullptr);
    if (rc) { printf("  rc %d\n", rc); return 1; }
    size_t bad = 0;
    if (combo == 0) {                                    // nothing in the epilogue: the plain forward, bit for bit
        float* y0 = al(ny, q.off);
        rc = vpn_conv2d_fwd(x, w, y0, B, Ci, Co, H, W, R, st, p, ws, wf, nullptr);
        if (rc) { printf("  conv2d_fwd rc %d\n", rc); return 1; }
        if (memcmp(y, y0, ny * 4)) { puts("  differs from vpn_conv2d_fwd"); ++bad; }
    }
    // ---- float64 restatement
    for (int b = 0; b < B; ++b) for (int co = 0; co < Co; ++co) for (int oh = 0; oh < OH; ++oh) for (int ow = 0; ow < OW; ++ow) {
        const size_t o = (((size_t)b * Co + co) * OH + oh) * OW + ow;
        double v = 0.0;
        for (int ci = 0; ci < Ci; ++ci) for (int r = 0; r < R; ++r) for (int s = 0; s < R; ++s) {
            const int ih = oh * st + r - p, iw = ow * st + s - p;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            v += (double)x[(((size_t)b * Ci + ci) * H + ih) * W + iw] * w[(((size_t)co * Ci + ci) * R + r) * R + s];
        }
        if (use_bias) v += bias[co];
        if (use_res) v += res[o];
        if (relu && v < 0) v = 0;
        bad += !((double)y[o] == v);                     // a NaN left behind differs
    }
    if (bad) printf("  combination %d: %zu elements differ\n", combo, bad);
    return bad != 0;
}

int main(int argc, char** argv) {          // an argument: only the shapes whose description contains it
    const Shape shapes[] = {
        {1, 1, 1, 1, 1, 1, 2, 0, false, "one pixel, one chunk: unsplit"},
        {1, 1, 1, 1, 1, 3, 2, 1, false, "image smaller than the kernel"},
        {1, 2, 3, 2, 2, 7, 2, 3, false, "OH = 1 with most taps in the padding"},
        {2, 3, 5, 9, 11, 7, 2, 3, true, "7x7, odd everything; misaligned"},
        {2, 5, 7, 6, 5, 3, 2, 1, false, "one tile, split, tails everywhere; 126 elements: the element merge"},
        {4, 5, 7, 6, 5, 3, 2, 1, false, "252 elements, 9 pixels a channel: a float4 of the merge holds two channels"},
        {4, 5, 7, 6, 5, 3, 2, 1, true, "the same, misaligned: the element merge"},
        {2, 6, 7, 8, 8, 1, 2, 0, false, "a 1x1 downsample, one chunk: unsplit"},
        {2, 40, 7, 8, 8, 1, 2, 0, false, "a 1x1 downsample of 40 channels, three chunks: split"},
        {1, 4, 65, 16, 16, 3, 2, 1, false, "N = 64 and M = 65: the tile edges"},
        {3, 19, 33, 7, 9, 3, 3, 0, true, "stride 3, tails in M, N and K; misaligned"},
        {1, 3, 130, 2, 67, 7, 1, 5, false, "padding wider than the image edge, three tiles along M"},
        {2, 5, 7, 5, 3, 3, 1, 1, false, "3x3, stride 1, padding 1"},
        {1, 2, 2, 128, 128, 3, 1, 1, false, "256 tiles of pixels, 3x3: unsplit"},
        {1, 1, 2, 128, 128, 7, 1, 3, false, "256 tiles of pixels, 7x7: unsplit"},
    };
    int bad = 0;
    for (const Shape& s : shapes) {
        if (argc > 1 && !strstr(s.what, argv[1])) continue;
        const bool large = (long long)s.B * s.Co * s.H * s.W > 20000;
        int b = 0;
        for (int combo = 0; combo < 8; ++combo) {
            if (large && combo != 0 && combo != 7) continue;
            b += run(s, combo);
        }
        printf("(%d,%3d,%4d,%3d,%3d, R %d, stride %d, pad %d) %-84s %s\n", s.B, s.Ci, s.Co, s.H, s.W, s.R, s.st, s.p, s.what, b ? "FAILED" : "exact");
        fflush(stdout);
        bad += b != 0;
    }
    if (argc == 1) {
        for (int R : {1, 3, 7}) {
            printf("R %d  unsplit calls %d, split calls %d\n", R, regimes[R][0], regimes[R][1]);
            bad += !regimes[R][0] || !regimes[R][1];
        }
        printf("split calls whose float4s hold two channels: %d\n", vec_straddle);
        bad += !vec_straddle;
    }
    {   // validation without a launch: vpn_conv2d_fwd's rejections with its codes, and relu
        float v[4] = {0, 0, 0, 0};
        auto f = [&](const float* x, const float* w, float* y, int B, int Ci, int Co, int H, int W, int R, int st, int p, int relu, void* ws, size_t n) {
            return vpn_conv2d_bias_act_fwd(x, w, nullptr, nullptr, y, B, Ci, Co, H, W, R, st, p, relu, ws, n, nullptr);
        };
        const int ok = f(nullptr, v, v, 1, 1, 1, 1, 1, 1, 1, 0, 0, nullptr, 0) == VPN_E_BADARG &&
                       f(v, nullptr, v, 1, 1, 1, 1, 1, 1, 1, 0, 0, nullptr, 0) == VPN_E_BADARG &&
                       f(v, v, nullptr, 1, 1, 1, 1, 1, 1, 1, 0, 0, nullptr, 0) == VPN_E_BADARG &&
                       f(v, v, v, 0, 1, 1, 1, 1, 1, 1, 0, 0, nullptr, 0) == VPN_E_BADARG &&
                       f(v, v, v, 1, 1, 1, 1, 1, 5, 1, 2, 0, nullptr, 0) == VPN_E_BADARG &&           // R = 5
                       f(v, v, v, 1, 1, 1, 1, 1, 1, 0, 0, 0, nullptr, 0) == VPN_E_BADARG &&           // stride 0
                       f(v, v, v, 1, 1, 1, 1, 1, 1, 1, -1, 0, nullptr, 0) == VPN_E_BADARG &&          // pad -1
                       f(v, v, v, 1, 1, 1, 2, 2, 3, 1, 0, 0, nullptr, 0) == VPN_E_BADARG &&           // H + 2p < R
                       f(v, v, v, 1, 1, 1, 1, 1, 1, 1, 0, 2, nullptr, 0) == VPN_E_BADARG &&           // relu 2
                       f(v, v, v, 1, 1, 1, 1, 1, 1, 1, 0, -1, nullptr, 0) == VPN_E_BADARG &&          // relu -1
                       f(v, v, v, 2, 5, 7, 5, 3, 3, 1, 1, 1, nullptr, 0) == VPN_E_BADARG &&           // split: no workspace
                       f(v, v, v, 2, 5, 7, 5, 3, 3, 1, 1, 1, v, 16) == VPN_E_BADARG &&                // too small
                       f(v, v, v, 2, 5, 7, 5, 3, 3, 1, 1, 1, (char*)v + 4, 1 << 20) == VPN_E_BADARG && // misaligned
                       f(v, v, v, 1 << 16, 1, 1, 1 << 8, 1 << 7, 1, 1, 0, 1, v, 16) == VPN_E_TOOBIG &&
                       f(v, v, v, 1, 1, 65536 * 64, 1, 1, 1, 1, 0, 1, v, 16) == VPN_E_TOOBIG;
        printf("%-48s %s\n", "argument validation", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
