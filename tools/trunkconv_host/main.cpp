// Host check of csrc/trunkconv.hip and csrc/trunkstride.hip (and the tile loop, merge and plan of csrc/vpn_conv_gemm.h that
// both use) without a GPU, in the manner of tools/fcstack_host and tools/trunknorm_host: the kernels' own source is compiled
// as C++ against that shim (a launch runs workgroup by workgroup on std::threads, one per work-item, real barriers, the
// f32-input MFMA builtin emulated through the per-wave exchange buffers with the instruction's lane maps and its k-ordered
// fmaf chain), and vpn_conv3x3_fwd / _bwd and vpn_conv2d_fwd / _bwd are compared with one float64 loop.  The inputs are
// small integers, so every product and partial sum is exact in fp32 and the results must EQUAL the float64 ones.  Every
// buffer has its exact size, so AddressSanitizer sees any access past an end; y, dx and dw are filled with NaN before the
// call, so an element the kernels forgot to write (an input pixel that no output reads) is caught.  Shapes of the 3x3
// entries: one pixel, H or W of 1, tails in all three GEMM dimensions, image rows and batch rows that cross tile edges; of
// the general entries: one pixel, an image smaller than the kernel, OH = 1 with most taps in the padding, odd sizes,
// even / odd H and W under stride 2, unread last rows and columns under 1x1 / 2, K = 147, the tile edges, stride 3,
// stride 1; of both: the split and the unsplit regime of every product, dx / dw NULL in turn, pointers 4 bytes past a
// 16-byte boundary (the merge's element path).
// It checks indexing, masking, barriers, the operand maps and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/trunkconv_host/main.cpp -o tc_host
//   ASAN_OPTIONS=detect_leaks=0 ./tc_host          (the check leaks its buffers on purpose: it exits right after)
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
#include "../../volumetric-primitives-net_amd/csrc/trunkconv.hip"
#include "../../volumetric-primitives-net_amd/csrc/trunkstride.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cmath>
#include <cstdio>
#include <random>
static std::mt19937 rng(1);
static float ri(int a) { return (float)std::uniform_int_distribution<int>(-a, a)(rng); }
// n floats that end where their allocation ends, filled with NaN; `off`: begin 4 bytes past a 16-byte boundary
static float* al(size_t n, bool off) {
    float* p = (float*)malloc((n + (off ? 1 : 0)) * 4) + (off ? 1 : 0);
    for (size_t i = 0; i < n; ++i) p[i] = NAN;
    return p;
}
static size_t differ(const float* got, const std::vector<double>& want) {
    size_t d = 0;
    for (size_t i = 0; i < want.size(); ++i) d += !((double)got[i] == want[i]);          // a NaN left behind differs
    return d;
}

enum { F3X3 = 0, F2D = 1 };        // the entry family a shape calls: vpn_conv3x3_* (R, st, p are 3, 1, 1) or vpn_conv2d_*
static int regimes[2][3][2];       // [family][product][split]: calls seen

struct Shape { int fam, B, Ci, Co, H, W, R, st, p; bool off; const char* what; };

static int splits(const Shape& q, int product) {
    return q.fam == F3X3 ? vpn_conv3x3_splits(q.B, q.Ci, q.Co, q.H, q.W, product)
                         : vpn_conv2d_splits(q.B, q.Ci, q.Co, q.H, q.W, q.R, q.st, q.p, product);
}
static size_t workspace(const Shape& q, int products) {
    return q.fam == F3X3 ? vpn_conv3x3_workspace(q.B, q.Ci, q.Co, q.H, q.W, products)
                         : vpn_conv2d_workspace(q.B, q.Ci, q.Co, q.H, q.W, q.R, q.st, q.p, products);
}

// skip: 0 both gradients, 1 dx only, 2 dw only
static int run(const Shape& q, int skip) {
    const int B = q.B, Ci = q.Ci, Co = q.Co, H = q.H, W = q.W, R = q.R, st = q.st, p = q.p;
    const bool off = q.off;
    const int OH = (H + 2 * p - R) / st + 1, OW = (W + 2 * p - R) / st + 1;
    const size_t nx = (size_t)B * Ci * H * W, ny = (size_t)B * Co * OH * OW, nw = (size_t)Co * Ci * R * R;
    float *x = al(nx, off), *w = al(nw, off), *y = al(ny, off), *dy = al(ny, off);
    for (size_t i = 0; i < nx; ++i) x[i] = ri(3);
    for (size_t i = 0; i < nw; ++i) w[i] = ri(2);
    for (size_t i = 0; i < ny; ++i) dy[i] = ri(2);
    const int products[3] = {VPN_CONV_FWD, VPN_CONV_DX, VPN_CONV_DW};
    for (int k = 0; k < 3; ++k) {
        const int S = splits(q, products[k]);
        if (S < 1) { printf("  splits %d\n", S); return 1; }
        if (k == 0 || (k == 1 && skip != 2) || (k == 2 && skip != 1)) ++regimes[q.fam][k][S > 1];
        const size_t out = k == 0 ? ny : k == 1 ? nx : nw;
        if (workspace(q, products[k]) != (S > 1 ? S * out * 4 : 0)) { puts("  workspace size and regime disagree"); return 1; }
    }
    const size_t wf = workspace(q, VPN_CONV_FWD);
    const size_t wb = workspace(q, skip == 1 ? VPN_CONV_DX : skip == 2 ? VPN_CONV_DW : VPN_CONV_DX | VPN_CONV_DW);
    void *wsf = nullptr, *wsb = nullptr;                 // 16-byte aligned, exact size
    if ((wf && posix_memalign(&wsf, 16, wf)) || (wb && posix_memalign(&wsb, 16, wb))) { puts("  no memory"); return 1; }
    int rc = q.fam == F3X3 ? vpn_conv3x3_fwd(x, w, y, B, Ci, Co, H, W, wsf, wf, nullptr)
                           : vpn_conv2d_fwd(x, w, y, B, Ci, Co, H, W, R, st, p, wsf, wf, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    float *dx = skip == 2 ? nullptr : al(nx, off), *dw = skip == 1 ? nullptr : al(nw, off);
    rc = q.fam == F3X3 ? vpn_conv3x3_bwd(dy, x, w, dx, dw, B, Ci, Co, H, W, wsb, wb, nullptr)
                       : vpn_conv2d_bwd(dy, x, w, dx, dw, B, Ci, Co, H, W, R, st, p, wsb, wb, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    // ---- float64 restatement
    std::vector<double> Y(ny, 0.0), DX(nx, 0.0), DW(nw, 0.0);
    for (int b = 0; b < B; ++b) for (int co = 0; co < Co; ++co) for (int oh = 0; oh < OH; ++oh) for (int ow = 0; ow < OW; ++ow) {
        const size_t o = (((size_t)b * Co + co) * OH + oh) * OW + ow;
        for (int ci = 0; ci < Ci; ++ci) for (int r = 0; r < R; ++r) for (int s = 0; s < R; ++s) {
            const int ih = oh * st + r - p, iw = ow * st + s - p;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            const size_t xi = (((size_t)b * Ci + ci) * H + ih) * W + iw, wi = (((size_t)co * Ci + ci) * R + r) * R + s;
            Y[o] += (double)x[xi] * w[wi];
            DX[xi] += (double)dy[o] * w[wi];
            DW[wi] += (double)dy[o] * x[xi];
        }
    }
    size_t bad = differ(y, Y);
    if (dx) bad += differ(dx, DX);
    if (dw) bad += differ(dw, DW);
    if (bad) printf("  %zu elements differ\n", bad);
    return bad != 0;
}

int main(int argc, char** argv) {          // an argument: only the shapes whose description contains it
    const Shape shapes[] = {
        {F3X3, 1, 1, 1, 1, 1, 3, 1, 1, false, "one pixel, one channel: only the centre tap exists"},
        {F3X3, 2, 5, 7, 5, 3, 3, 1, 1, false, "odd everything, one tile"},
        {F3X3, 3, 19, 33, 7, 9, 3, 1, 1, true, "tails in M, N and K; batch rows cross the tile edge; misaligned"},
        {F3X3, 1, 3, 130, 2, 67, 3, 1, 1, false, "three tiles along M, image rows cross tile edges"},
        {F3X3, 2, 70, 6, 1, 33, 3, 1, 1, false, "H = 1: no row above or below"},
        {F3X3, 2, 6, 70, 33, 1, 3, 1, 1, true, "W = 1: no column left or right; misaligned"},
        {F3X3, 1, 8, 64, 8, 8, 3, 1, 1, false, "C_out, 9 C_in and B H W at the tile: 64, 72, 64"},
        {F3X3, 1, 7, 65, 5, 13, 3, 1, 1, false, "one past the tile: 65, 63, 65"},
        {F3X3, 1, 2, 17, 1, 17, 3, 1, 1, false, "around the chunk: 17, 18, 17"},
        {F3X3, 1, 2, 2, 128, 128, 3, 1, 1, false, "256 tiles of pixels: forward and data gradient unsplit by the tile rule, weight gradient 32 slices"},
        {F3X3, 1, 114, 1024, 3, 6, 3, 1, 1, false, "16 x 17 tiles of weights: the weight gradient unsplit by the tile rule"},
        {F2D, 1, 1, 1, 1, 1, 1, 2, 0, false, "one pixel"},
        {F2D, 1, 1, 1, 1, 1, 3, 2, 1, false, "image smaller than the kernel"},
        {F2D, 1, 2, 3, 2, 2, 7, 2, 3, false, "OH = 1 with most taps in the padding"},
        {F2D, 2, 3, 5, 9, 11, 7, 2, 3, true, "odd everything; misaligned"},
        {F2D, 2, 5, 7, 6, 5, 3, 2, 1, false, "even H, odd W"},
        {F2D, 2, 5, 7, 5, 6, 3, 2, 1, true, "odd H, even W; misaligned"},
        {F2D, 2, 6, 7, 8, 8, 1, 2, 0, false, "last row and column unread: dx is 0 there"},
        {F2D, 1, 3, 64, 16, 16, 7, 2, 3, false, "K = 147: nine chunks and a tail of 3"},
        {F2D, 1, 4, 65, 16, 16, 3, 2, 1, false, "N = 64 and M = 65: the tile edges"},
        {F2D, 3, 19, 33, 7, 9, 3, 3, 0, true, "stride 3; misaligned"},
        {F2D, 2, 5, 7, 5, 3, 3, 1, 1, false, "3x3, stride 1, padding 1"},
        {F2D, 2, 5, 7, 5, 3, 1, 1, 0, false, "1x1, stride 1"},
        {F2D, 1, 37, 1024, 3, 6, 7, 2, 3, false, "16 x 29 tiles of weights: the weight gradient unsplit by the tile rule"},
        {F2D, 1, 2, 2, 256, 256, 1, 2, 0, false, "256 tiles of output pixels: forward unsplit; data gradient 1024 tiles"},
    };
    const char* fams[2] = {"conv3x3", "conv2d"};
    int bad = 0, n[2] = {0, 0};
    for (const Shape& s : shapes) {
        if (argc > 1 && !strstr(s.what, argv[1])) continue;
        int b = 0;
        for (int skip = 0; skip < 3; ++skip) {
            if ((long long)s.B * s.Ci * s.Co * s.H * s.W > 200000 && skip != (n[s.fam] % 3)) continue;       // the large ones: one variant each
            b += run(s, skip);
        }
        ++n[s.fam];
        printf("%-7s (%d,%3d,%4d,%3d,%3d, R %d, stride %d, pad %d) %-100s %s\n", fams[s.fam], s.B, s.Ci, s.Co, s.H, s.W, s.R, s.st, s.p, s.what,
               b ? "FAILED" : "exact");
        fflush(stdout);
        bad += b != 0;
    }
    if (argc == 1) {
        const char* names[3] = {"forward", "data gradient", "weight gradient"};
        for (int f = 0; f < 2; ++f) for (int p = 0; p < 3; ++p) {
            printf("%-7s %-16s unsplit calls %d, split calls %d\n", fams[f], names[p], regimes[f][p][0], regimes[f][p][1]);
            bad += !regimes[f][p][0] || !regimes[f][p][1];
        }
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0};
        int ok = vpn_conv3x3_fwd(nullptr, v, v, 1, 1, 1, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_fwd(v, nullptr, v, 1, 1, 1, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_fwd(v, v, nullptr, 1, 1, 1, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_fwd(v, v, v, 0, 1, 1, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_fwd(v, v, v, 1, 1, 1, -1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_fwd(v, v, v, 2, 5, 7, 5, 3, nullptr, 0, nullptr) == VPN_E_BADARG &&          // split: no workspace
                 vpn_conv3x3_fwd(v, v, v, 2, 5, 7, 5, 3, v, 16, nullptr) == VPN_E_BADARG &&               // too small
                 vpn_conv3x3_fwd(v, v, v, 2, 5, 7, 5, 3, (char*)v + 4, 1 << 20, nullptr) == VPN_E_BADARG && // misaligned
                 vpn_conv3x3_fwd(v, v, v, 1 << 16, 1, 1, 1 << 8, 1 << 7, v, 16, nullptr) == VPN_E_TOOBIG &&
                 vpn_conv3x3_fwd(v, v, v, 1, 1, 65536 * 64, 1, 1, v, 16, nullptr) == VPN_E_TOOBIG &&
                 vpn_conv3x3_bwd(nullptr, v, v, v, v, 1, 1, 1, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_bwd(v, v, v, v, nullptr, 2, 5, 7, 5, 3, nullptr, 0, nullptr) == VPN_E_BADARG &&
                 vpn_conv3x3_bwd(v, v, v, nullptr, nullptr, 2, 5, 7, 5, 3, nullptr, 0, nullptr) == 0 &&
                 vpn_conv3x3_workspace(0, 1, 1, 1, 1, 7) == 0 && vpn_conv3x3_workspace(1, 2, 2, 128, 128, VPN_CONV_FWD) == 0;
        printf("%-48s %s\n", "conv3x3 argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
        ok = vpn_conv2d_fwd(nullptr, v, v, 1, 1, 1, 1, 1, 1, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_fwd(v, nullptr, v, 1, 1, 1, 1, 1, 1, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_fwd(v, v, nullptr, 1, 1, 1, 1, 1, 1, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_fwd(v, v, v, 0, 1, 1, 1, 1, 1, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_fwd(v, v, v, 1, 1, 1, -1, 1, 1, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_fwd(v, v, v, 1, 1, 1, 1, 1, 5, 1, 2, nullptr, 0, nullptr) == VPN_E_BADARG &&           // R = 5
             vpn_conv2d_fwd(v, v, v, 1, 1, 1, 1, 1, 1, 0, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&           // stride 0
             vpn_conv2d_fwd(v, v, v, 1, 1, 1, 1, 1, 1, 1, -1, nullptr, 0, nullptr) == VPN_E_BADARG &&          // pad -1
             vpn_conv2d_fwd(v, v, v, 1, 1, 1, 2, 2, 3, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&           // H + 2p < R
             vpn_conv2d_fwd(v, v, v, 2, 5, 7, 5, 3, 3, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&           // split: no workspace
             vpn_conv2d_fwd(v, v, v, 2, 5, 7, 5, 3, 3, 1, 1, v, 16, nullptr) == VPN_E_BADARG &&                // too small
             vpn_conv2d_fwd(v, v, v, 2, 5, 7, 5, 3, 3, 1, 1, (char*)v + 4, 1 << 20, nullptr) == VPN_E_BADARG && // misaligned
             vpn_conv2d_fwd(v, v, v, 1 << 16, 1, 1, 1 << 8, 1 << 7, 1, 1, 0, v, 16, nullptr) == VPN_E_TOOBIG &&
             vpn_conv2d_fwd(v, v, v, 1, 1, 65536 * 64, 1, 1, 1, 1, 0, v, 16, nullptr) == VPN_E_TOOBIG &&
             vpn_conv2d_bwd(nullptr, v, v, v, v, 1, 1, 1, 1, 1, 1, 1, 0, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_bwd(v, v, v, v, nullptr, 2, 5, 7, 5, 3, 3, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
             vpn_conv2d_bwd(v, v, v, nullptr, nullptr, 2, 5, 7, 5, 3, 3, 1, 1, nullptr, 0, nullptr) == 0 &&
             vpn_conv2d_workspace(0, 1, 1, 1, 1, 1, 1, 0, 7) == 0 && vpn_conv2d_workspace(1, 2, 2, 256, 256, 1, 2, 0, VPN_CONV_FWD) == 0;
        printf("%-48s %s\n", "conv2d argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
