// Host check of csrc/trunkconv.hip without a GPU, in the manner of tools/fcstack_host and tools/trunknorm_host: the kernels'
// own source is compiled as C++ against that shim (a launch runs workgroup by workgroup on std::threads, one per work-item,
// real barriers, the two f32-input MFMA builtins emulated through the per-wave exchange buffers with the instruction's lane
// maps and its k-ordered fmaf chain), and vpn_conv3x3_fwd / _bwd are compared with a float64 loop.  The inputs are small
// integers, so every product and partial sum is exact in fp32 and the results must EQUAL the float64 ones.  Every buffer
// has its exact size, so AddressSanitizer sees any access past an end: one pixel, H or W of 1, tails in all three GEMM
// dimensions, image rows and batch rows that cross tile edges, the split and the unsplit regime of every product, dx / dw
// NULL in turn, pointers 4 bytes past a 16-byte boundary (the merge's element path).
// It checks indexing, masking, barriers, the operand maps and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/trunkconv_host/main.cpp -o tc_host
//   ASAN_OPTIONS=detect_leaks=0 ./tc_host          (the check leaks its buffers on purpose: it exits right after)
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
#include "../../volumetric-primitives-net_amd/csrc/trunkconv.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cstdio>
#include <random>
static std::mt19937 rng(1);
static float ri(int a) { return (float)std::uniform_int_distribution<int>(-a, a)(rng); }
// n floats that end where their allocation ends; `off`: begin 4 bytes past a 16-byte boundary
static float* al(size_t n, bool off) { float* p = (float*)malloc((n + (off ? 1 : 0)) * 4); return off ? p + 1 : p; }
static size_t differ(const float* got, const std::vector<double>& want) {
    size_t d = 0;
    for (size_t i = 0; i < want.size(); ++i) d += (double)got[i] != want[i];
    return d;
}

static int regimes[3][2];          // [product][split]: calls seen

// skip: 0 both gradients, 1 dx only, 2 dw only
static int run(int B, int Ci, int Co, int H, int W, bool off, int skip) {
    const size_t HW = (size_t)H * W, nx = HW * B * Ci, ny = HW * B * Co, nw = (size_t)Co * Ci * 9;
    float *x = al(nx, off), *w = al(nw, off), *y = al(ny, off), *dy = al(ny, off);
    for (size_t i = 0; i < nx; ++i) x[i] = ri(3);
    for (size_t i = 0; i < nw; ++i) w[i] = ri(2);
    for (size_t i = 0; i < ny; ++i) dy[i] = ri(2);
    const int products[3] = {VPN_CONV_FWD, VPN_CONV_DX, VPN_CONV_DW};
    for (int p = 0; p < 3; ++p) {
        const int S = vpn_conv3x3_splits(B, Ci, Co, H, W, products[p]);
        if (S < 1) { printf("  splits %d\n", S); return 1; }
        if (p == 0 || (p == 1 && skip != 2) || (p == 2 && skip != 1)) ++regimes[p][S > 1];
        const size_t out = p == 0 ? ny : p == 1 ? nx : nw;
        if (vpn_conv3x3_workspace(B, Ci, Co, H, W, products[p]) != (S > 1 ? S * out * 4 : 0)) { puts("  workspace size and regime disagree"); return 1; }
    }
    const size_t wf = vpn_conv3x3_workspace(B, Ci, Co, H, W, VPN_CONV_FWD);
    const size_t wb = vpn_conv3x3_workspace(B, Ci, Co, H, W, skip == 1 ? VPN_CONV_DX : skip == 2 ? VPN_CONV_DW : VPN_CONV_DX | VPN_CONV_DW);
    void *wsf = nullptr, *wsb = nullptr;                 // 16-byte aligned, exact size
    if ((wf && posix_memalign(&wsf, 16, wf)) || (wb && posix_memalign(&wsb, 16, wb))) { puts("  no memory"); return 1; }
    int rc = vpn_conv3x3_fwd(x, w, y, B, Ci, Co, H, W, wsf, wf, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    float *dx = skip == 2 ? nullptr : al(nx, off), *dw = skip == 1 ? nullptr : al(nw, off);
    rc = vpn_conv3x3_bwd(dy, x, w, dx, dw, B, Ci, Co, H, W, wsb, wb, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    // ---- float64 restatement
    std::vector<double> Y(ny, 0.0), DX(nx, 0.0), DW(nw, 0.0);
    for (int b = 0; b < B; ++b) for (int co = 0; co < Co; ++co) for (int h = 0; h < H; ++h) for (int ww = 0; ww < W; ++ww) {
        const size_t o = (((size_t)b * Co + co) * H + h) * W + ww;
        for (int ci = 0; ci < Ci; ++ci) for (int r = 0; r < 3; ++r) for (int s = 0; s < 3; ++s) {
            const int ih = h + r - 1, iw = ww + s - 1;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            const size_t xi = (((size_t)b * Ci + ci) * H + ih) * W + iw, wi = (((size_t)co * Ci + ci) * 3 + r) * 3 + s;
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
    struct Shape { int B, Ci, Co, H, W; bool off; const char* what; };
    const Shape shapes[] = {
        {1, 1, 1, 1, 1, false, "one pixel, one channel: only the centre tap exists"},
        {2, 5, 7, 5, 3, false, "odd everything, one tile"},
        {3, 19, 33, 7, 9, true, "tails in M, N and K; batch rows cross the tile edge; misaligned"},
        {1, 3, 130, 2, 67, false, "three tiles along M, image rows cross tile edges"},
        {2, 70, 6, 1, 33, false, "H = 1: no row above or below"},
        {2, 6, 70, 33, 1, true, "W = 1: no column left or right; misaligned"},
        {1, 8, 64, 8, 8, false, "C_out, 9 C_in and B H W at the tile: 64, 72, 64"},
        {1, 7, 65, 5, 13, false, "one past the tile: 65, 63, 65"},
        {1, 2, 17, 1, 17, false, "around the chunk: 17, 18, 17"},
        {1, 2, 2, 128, 128, false, "256 tiles of pixels: forward and data gradient unsplit by the tile rule, weight gradient 32 slices"},
        {1, 114, 1024, 3, 6, false, "16 x 17 tiles of weights: the weight gradient unsplit by the tile rule"},
    };
    int bad = 0, n = 0;
    for (const Shape& s : shapes) {
        if (argc > 1 && !strstr(s.what, argv[1])) continue;
        int b = 0;
        for (int skip = 0; skip < 3; ++skip) {
            if (s.B * s.Ci * s.Co * s.H * s.W > 200000 && skip != (n % 3)) continue;       // the large ones: one variant each
            b += run(s.B, s.Ci, s.Co, s.H, s.W, s.off, skip);
        }
        ++n;
        printf("(%d,%3d,%3d,%3d,%3d) %-88s %s\n", s.B, s.Ci, s.Co, s.H, s.W, s.what, b ? "FAILED" : "exact");
        fflush(stdout);
        bad += b != 0;
    }
    if (argc == 1) {
        const char* names[3] = {"forward", "data gradient", "weight gradient"};
        for (int p = 0; p < 3; ++p) {
            printf("%-16s unsplit calls %d, split calls %d\n", names[p], regimes[p][0], regimes[p][1]);
            bad += !regimes[p][0] || !regimes[p][1];
        }
    }
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0};
        const int ok = vpn_conv3x3_fwd(nullptr, v, v, 1, 1, 1, 1, 1, nullptr, 0, nullptr) == VPN_E_BADARG &&
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
        printf("%-40s %s\n", "argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
