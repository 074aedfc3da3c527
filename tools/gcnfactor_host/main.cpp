// Host check of conv1 in factored form (the gcn_factored_ kernels of csrc/gcn.hip and the kernels they reuse)
// without a GPU, in the manner of tools/trunktail_host: the kernels' own source is compiled as C++ against the shim of
// tools/fcstack_host (a launch runs workgroup by workgroup on std::threads, one per work-item, real barriers), and
// vpn_gcn_factored_fwd / _bwd are compared with a float64 restatement of the PLAIN form: the row [encoding | pooled |
// global] of every vertex times Theta, the maps read NCHW.  The caller's dense products (the projected maps, g Theta_g) are
// plain loops here, as torch.matmul forms them in ops.py.  Checked: h, grad_proj (against the per-pixel weighted sums of the
// restatement), grad_theta_e (against x^T dh) and grad_verts (against central differences of the float64 loss, which go
// through the encoding, the grid and the min / max).  Every buffer has its exact size, so AddressSanitizer sees any access
// past an end.  Shapes: vertex counts that are no multiple of the 32-vertex and 16-vertex tiles, channel counts that end
// inside a 128-channel chunk and that need a second 512-channel pass, every encoding width, no maps, no global block, and
// bounds that put corners outside the maps.  It checks indexing, barriers and the host-side launch logic; it says nothing
// about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/gcnfactor_host/main.cpp -o gf_host
//   ./gf_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
using std::max;
inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
#include "../../volumetric-primitives-net_amd/csrc/gcn.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(7);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
static float uni() { return std::uniform_real_distribution<float>(-0.5f, 0.5f)(rng); }
static float* al(size_t n) { return (float*)malloc((n ? n : 1) * 4); }       // exact size: the allocation ends where the data ends

struct Case { int B, N, Cout, venc, L, C[4], H[4], W[4], G; bool wide; const char* what; };

struct Problem {
    Case c; int ctot, Sp;
    std::vector<float> verts, bounds, glob, theta, R; std::vector<float> map[4];
};

// float64 restatement of the plain form: rows x [B N, ctot] and, per (vertex, level), corners and weights
struct Corner { int pix[4]; double w[4]; };
static void plain_rows(const Problem& p, const std::vector<double>& v, std::vector<double>& x, std::vector<Corner>* corners) {
    const Case& c = p.c;
    x.assign((size_t)c.B * c.N * p.ctot, 0.0);
    if (corners) corners->assign((size_t)c.B * c.N * (c.L ? c.L : 1), Corner{{-1, -1, -1, -1}, {0, 0, 0, 0}});
    for (int b = 0; b < c.B; ++b) {
        double zmin = 1e300, zmax = -1e300, ymin = 1e300, ymax = -1e300;
        for (int i = 0; i < c.N; ++i) {
            const double* q = &v[((size_t)b * c.N + i) * 3];
            zmin = std::min(zmin, q[2]); zmax = std::max(zmax, q[2]); ymin = std::min(ymin, q[1]); ymax = std::max(ymax, q[1]);
        }
        for (int i = 0; i < c.N; ++i) {
            const double* q = &v[((size_t)b * c.N + i) * 3];
            double* row = &x[((size_t)b * c.N + i) * p.ctot];
            for (int k = 0; k < c.venc; ++k) {
                if (k < 3) row[k] = q[k];
                else { const int kk = (k - 3) / 3, d = (k - 3) % 3; const double a = q[d] * (double)(1 << (kk >> 1)); row[k] = (kk & 1) ? cos(a) : sin(a); }
            }
            int col = c.venc;
            for (int l = 0; l < c.L; ++l) {
                const double b0 = p.bounds[b * 4], b1 = p.bounds[b * 4 + 1], b2 = p.bounds[b * 4 + 2], b3 = p.bounds[b * 4 + 3];
                const double gx = b0 + (1 - (q[2] - zmin) / (zmax - zmin)) * (b1 - b0), gy = b2 + (1 - (q[1] - ymin) / (ymax - ymin)) * (b3 - b2);
                const int H = c.H[l], W = c.W[l], C = c.C[l];
                const double ix = (gx + 1) / 2 * (W - 1), iy = (gy + 1) / 2 * (H - 1);
                const int x0 = (int)floor(ix), y0 = (int)floor(iy);
                const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
                const double ws[4] = {(x0 + 1 - ix) * (y0 + 1 - iy), (ix - x0) * (y0 + 1 - iy), (x0 + 1 - ix) * (iy - y0), (ix - x0) * (iy - y0)};
                for (int k = 0; k < 4; ++k) {
                    if (xs[k] < 0 || xs[k] >= W || ys[k] < 0 || ys[k] >= H) continue;
                    const int pix = ys[k] * W + xs[k];
                    if (corners) { Corner& cr = (*corners)[((size_t)b * c.N + i) * c.L + l]; cr.pix[k] = pix; cr.w[k] = ws[k]; }
                    for (int ch = 0; ch < C; ++ch) row[col + ch] += ws[k] * (double)p.map[l][((size_t)b * C + ch) * H * W + pix];
                }
                col += C;
            }
            for (int k = 0; k < c.G; ++k) row[col + k] = p.glob[(size_t)b * c.G + k];
        }
    }
}

static double plain_loss(const Problem& p, const std::vector<double>& v) {
    std::vector<double> x; plain_rows(p, v, x, nullptr);
    const Case& c = p.c; double s = 0;
    for (size_t r = 0; r < (size_t)c.B * c.N; ++r)
        for (int k = 0; k < p.ctot; ++k) {
            const double xv = x[r * p.ctot + k]; if (xv == 0) continue;
            double d = 0; for (int o = 0; o < c.Cout; ++o) d += (double)p.theta[(size_t)k * c.Cout + o] * (double)p.R[r * c.Cout + o];
            s += xv * d;
        }
    return s;
}

static double cmp(const float* got, const std::vector<double>& want) {
    double m = 1e-30, d = 0;
    for (size_t i = 0; i < want.size(); ++i) { m = std::max(m, fabs(want[i])); d = std::max(d, fabs(want[i] - (double)got[i])); }
    return d / m;
}

static int run(const Case& c) {
    Problem p; p.c = c; p.Sp = 0; p.ctot = c.venc + c.G;
    for (int l = 0; l < c.L; ++l) { p.ctot += c.C[l]; p.Sp += c.H[l] * c.W[l]; }
    const size_t rows = (size_t)c.B * c.N;
    p.verts.resize(rows * 3); p.bounds.resize((size_t)c.B * 4); p.glob.resize((size_t)c.B * c.G); p.theta.resize((size_t)p.ctot * c.Cout); p.R.resize(rows * c.Cout);
    for (float& f : p.verts) f = uni();
    for (int b = 0; b < c.B; ++b) {
        const float in[4] = {-0.8f, 0.7f, -0.6f, 0.9f}, out[4] = {-1.3f, 1.2f, -0.9f, 1.4f};
        for (int k = 0; k < 4; ++k) p.bounds[b * 4 + k] = (c.wide ? out[k] : in[k]) + 0.01f * b;
    }
    for (float& f : p.glob) f = rnd();
    for (float& f : p.theta) f = 0.2f * rnd();
    for (float& f : p.R) f = rnd();
    for (int l = 0; l < c.L; ++l) { p.map[l].resize((size_t)c.B * c.C[l] * c.H[l] * c.W[l]); for (float& f : p.map[l]) f = rnd(); }
    int hw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = 0; l < c.L; ++l) { hw[2 * l] = c.H[l]; hw[2 * l + 1] = c.W[l]; }
#define HW hw[0], hw[1], hw[2], hw[3], hw[4], hw[5], hw[6], hw[7]
    // ---- the caller's part: theta_e = the first rows, proj = map (NHWC) Theta_l level after level, gtheta = g Theta_g
    const size_t pbytes = vpn_gcn_factored_proj_workspace(c.B, c.Cout, c.L, HW);
    if (pbytes != (size_t)c.B * p.Sp * c.Cout * 4) { puts("  proj workspace size"); return 1; }
    float *verts = al(rows * 3), *bounds = al((size_t)c.B * 4), *theta_e = al((size_t)c.venc * c.Cout), *proj = al(pbytes / 4), *gth = c.G ? al((size_t)c.B * c.Cout) : nullptr;
    float *R = al(rows * c.Cout);
    memcpy(verts, p.verts.data(), rows * 12); memcpy(bounds, p.bounds.data(), (size_t)c.B * 16); memcpy(theta_e, p.theta.data(), (size_t)c.venc * c.Cout * 4);
    memcpy(R, p.R.data(), rows * c.Cout * 4);
    {
        int row0 = c.venc; size_t p0 = 0;
        for (int l = 0; l < c.L; ++l) {
            const int n = c.H[l] * c.W[l];
            for (int b = 0; b < c.B; ++b) for (int px = 0; px < n; ++px) for (int o = 0; o < c.Cout; ++o) {
                float s = 0;
                for (int ch = 0; ch < c.C[l]; ++ch) s += p.map[l][((size_t)b * c.C[l] + ch) * n + px] * p.theta[(size_t)(row0 + ch) * c.Cout + o];
                proj[((size_t)b * p.Sp + p0 + px) * c.Cout + o] = s;
            }
            row0 += c.C[l]; p0 += n;
        }
        for (int b = 0; b < c.B && c.G; ++b) for (int o = 0; o < c.Cout; ++o) {
            float s = 0;
            for (int k = 0; k < c.G; ++k) s += p.glob[(size_t)b * c.G + k] * p.theta[(size_t)(row0 + k) * c.Cout + o];
            gth[(size_t)b * c.Cout + o] = s;
        }
    }
    float *ext = al((size_t)c.B * 4), *grid = al(rows * 2), *h = al(rows * c.Cout); int32_t* ext_idx = (int32_t*)al((size_t)c.B * 4);
    int rc = vpn_gcn_factored_fwd(verts, bounds, gth, c.venc ? theta_e : nullptr, c.L ? proj : nullptr, c.B, c.N, c.Cout, c.venc, c.L, HW,
                                  ext, ext_idx, grid, h, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    // ---- float64, plain form
    std::vector<double> v64(p.verts.begin(), p.verts.end()), x; std::vector<Corner> corners;
    plain_rows(p, v64, x, &corners);
    std::vector<double> H64(rows * c.Cout, 0.0), dTe((size_t)c.venc * c.Cout, 0.0), dP((size_t)c.B * p.Sp * c.Cout, 0.0);
    size_t outside = 0;
    for (size_t r = 0; r < rows; ++r) {
        for (int k = 0; k < p.ctot; ++k) {
            const double xv = x[r * p.ctot + k]; if (xv == 0) continue;
            for (int o = 0; o < c.Cout; ++o) H64[r * c.Cout + o] += xv * (double)p.theta[(size_t)k * c.Cout + o];
        }
        for (int k = 0; k < c.venc; ++k) for (int o = 0; o < c.Cout; ++o) dTe[(size_t)k * c.Cout + o] += x[r * p.ctot + k] * (double)p.R[r * c.Cout + o];
        size_t p0 = 0;
        for (int l = 0; l < c.L; ++l) {
            const Corner& cr = corners[r * c.L + l];
            for (int k = 0; k < 4; ++k) {
                if (cr.pix[k] < 0) { ++outside; continue; }
                for (int o = 0; o < c.Cout; ++o) dP[((r / c.N) * p.Sp + p0 + cr.pix[k]) * c.Cout + o] += cr.w[k] * (double)p.R[r * c.Cout + o];
            }
            p0 += c.H[l] * c.W[l];
        }
    }
    double worst = cmp(h, H64);
    // ---- backward: everything wanted, then each output alone (the others NULL)
    const size_t wsb = vpn_gcn_factored_bwd_workspace(c.B, c.N, c.Cout, c.venc, c.L, HW);
    void* ws = malloc(wsb ? wsb : 1);
    float *gv = al(rows * 3), *gp = al(pbytes / 4), *gte = al((size_t)c.venc * c.Cout);
    rc = vpn_gcn_factored_bwd(R, verts, bounds, c.venc ? theta_e : nullptr, c.L ? proj : nullptr, c.B, c.N, c.Cout, c.venc, c.L, HW, ext, ext_idx,
                              grid, ws, gv, c.L ? gp : nullptr, c.venc ? gte : nullptr, nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    if (c.L) worst = std::max(worst, cmp(gp, dP));
    if (c.venc) worst = std::max(worst, cmp(gte, dTe));
    {
        std::vector<double> dV(rows * 3);
        const double eps = 1e-6;
        for (size_t i = 0; i < rows * 3; ++i) {
            std::vector<double> a(v64), b(v64); a[i] += eps; b[i] -= eps;
            dV[i] = (plain_loss(p, a) - plain_loss(p, b)) / (2 * eps);
        }
        worst = std::max(worst, cmp(gv, dV));
    }
    int bad = 0;
    for (int only = 0; only < 3; ++only) {
        float *gv2 = al(rows * 3), *gp2 = al(pbytes / 4), *gte2 = al((size_t)c.venc * c.Cout);
        rc = vpn_gcn_factored_bwd(R, verts, bounds, c.venc ? theta_e : nullptr, c.L ? proj : nullptr, c.B, c.N, c.Cout, c.venc, c.L, HW, ext, ext_idx,
                                  grid, ws, only == 0 ? gv2 : nullptr, only == 1 && c.L ? gp2 : nullptr, only == 2 && c.venc ? gte2 : nullptr, nullptr);
        if (rc || (only == 0 && memcmp(gv, gv2, rows * 12)) || (only == 1 && c.L && memcmp(gp, gp2, pbytes)) ||
            (only == 2 && c.venc && memcmp(gte, gte2, (size_t)c.venc * c.Cout * 4))) { printf("  output %d alone differs\n", only); ++bad; }
    }
    const double tol = 2e-5;           // fp32 against float64
    size_t all = rows * 4 * (c.L ? c.L : 1);
    printf("B %d N %3d Cout %3d venc %2d L %d G %2d  %-58s corners outside %4.1f%%  worst rel err %.2e  %s\n", c.B, c.N, c.Cout, c.venc, c.L, c.G, c.what,
           c.L ? 100.0 * outside / all : 0.0, worst, bad || worst > tol ? "FAILED" : "ok");
    if (c.wide && (outside * 10 < all || outside * 10 > all * 9)) { puts("  the wide bounds leave too few corners inside or outside"); ++bad; }
    return bad || worst > tol;
#undef HW
}

int main(int argc, char** argv) {          // an argument: only the cases whose description contains it
    const Case cases[] = {
        {2, 70, 136, 39, 2, {5, 3, 0, 0}, {5, 3, 0, 0}, {7, 2, 0, 0}, 4, false, "tiles and chunks with a remainder"},
        {2, 70, 136, 39, 2, {5, 3, 0, 0}, {5, 3, 0, 0}, {7, 2, 0, 0}, 4, true, "the same, corners outside the maps"},
        {1, 33, 8, 3, 4, {2, 3, 4, 5}, {8, 4, 2, 1}, {8, 4, 2, 1}, 0, false, "venc = 3, four levels down to 1 x 1, no global block"},
        {2, 16, 12, 0, 1, {6, 0, 0, 0}, {4, 0, 0, 0}, {6, 0, 0, 0}, 3, true, "venc = 0, one level"},
        {2, 40, 24, 39, 0, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, 5, false, "no maps: encoding and global only"},
        {1, 20, 520, 39, 1, {3, 0, 0, 0}, {3, 0, 0, 0}, {3, 0, 0, 0}, 2, false, "Cout = 520: a second 512-channel pass"},
    };
    int bad = 0;
    for (const Case& c : cases) {
        if (argc > 1 && !strstr(c.what, argv[1])) continue;
        bad += run(c);
    }
    {   // validation without a launch
        alignas(16) float v[4] = {0, 0, 0, 0}; int32_t i4[4];
        const int ok = vpn_gcn_factored_fwd(v, v, nullptr, v, v, 1, 1, 6, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr) == VPN_E_BADARG &&     // Cout % 4
                       vpn_gcn_factored_fwd(v, v, nullptr, v, v, 1, 1, 4, 5, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr) == VPN_E_BADARG &&     // venc
                       vpn_gcn_factored_fwd(v, v, nullptr, v, v, 1, 1, 4, 3, 5, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr) == VPN_E_BADARG &&     // L
                       vpn_gcn_factored_fwd(v, v, nullptr, nullptr, v, 1, 1, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr) == VPN_E_BADARG && // theta_e
                       vpn_gcn_factored_fwd(v, v, nullptr, v, nullptr, 1, 1, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr) == VPN_E_BADARG && // proj
                       vpn_gcn_factored_fwd(v, v, nullptr, v, v, 0, 1, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_factored_bwd(nullptr, v, v, v, v, 1, 1, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, v, v, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_factored_bwd(v, v, v, v, v, 1, 1, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, nullptr, v, v, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_factored_bwd(v, v, v, v, v, 1, 8193, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, v, nullptr, v, nullptr, nullptr) == VPN_E_TOOBIG &&
                       vpn_gcn_factored_bwd(v, v, v, v, v, 1, 1, 4, 3, 1, 1, 1, 0, 0, 0, 0, 0, 0, v, i4, v, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 &&
                       vpn_gcn_factored_proj_workspace(2, 8, 2, 3, 4, 2, 2, 0, 0, 0, 0) == 2 * 16 * 8 * 4 && vpn_gcn_factored_proj_workspace(2, 6, 1, 3, 4, 0, 0, 0, 0, 0, 0) == 0 &&
                       vpn_gcn_factored_bwd_workspace(2, 100, 8, 39, 1, 3, 4, 0, 0, 0, 0, 0, 0) == (2 * 100 * 4 + 2 * (4 * 5 + 2) + 2 * 100 * 2 + 2 * 39 * 8) * 4 &&
                       vpn_gcn_factored_bwd_workspace(2, 100, 8, 5, 1, 3, 4, 0, 0, 0, 0, 0, 0) == 0;
        printf("%-85s %s\n", "argument validation and workspace size", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
