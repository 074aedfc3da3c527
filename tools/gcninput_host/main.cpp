// Host check of the plain GCN input path (vpn_gcn_input_fwd / _bwd, vpn_gcn_bounds, vpn_gcn_aggregate, vpn_gcn_colsum of
// csrc/gcn.hip) without a GPU, in the manner of tools/gcnfactor_host: the kernels' own source is compiled as
// C++ against the shim of tools/fcstack_host (a launch runs workgroup by workgroup on std::threads, one per work-item, real
// barriers) and compared with a float64 restatement written here: the row [encoding | pooled | global] of every vertex, the
// maps read NCHW.  Checked: the rows, the map gradients (against the per-pixel weighted sums of the restatement), the column
// sum that is the global block's gradient, and grad_verts against central differences of the float64 loss, which go through
// the encoding, the grid and the min / max.  In the restatement an extent is the coordinate of the LOWEST vertex index that
// holds it in the unperturbed data: without ties that is the plain min / max, with ties it is the rule of torch.max /
// torch.min, which the kernels follow.  vpn_gcn_input_bwd runs with every output, with grad_verts alone and with the map
// gradients alone; the partial calls must reproduce the full one bit for bit.  Every buffer has its exact size, so
// AddressSanitizer sees any access past an end.  Shapes: non-square levels down to 1 x 1, C = 65 (a second 64-lane chunk
// with one live lane), N = 2, 70 and 130 (no multiple of the 4 rows of a vertex workgroup; 140 rows cross a sample inside
// one), tied extents, empty-image bounds (vertices exactly on ix = W - 1), bounds that put corners outside the maps, no maps,
// no encoding.
// It checks indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/gcninput_host/main.cpp -o gi_host
//   ./gi_host
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
static std::mt19937 rng(11);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
static float uni() { return std::uniform_real_distribution<float>(-0.5f, 0.5f)(rng); }
static float* al(size_t n) { return (float*)malloc((n ? n : 1) * 4); }       // exact size: the allocation ends where the data ends
static float* al(const std::vector<float>& v) { float* p = al(v.size()); memcpy(p, v.data(), v.size() * 4); return p; }

enum Bounds { INSIDE, WIDE, EMPTY_IMAGE };
struct Case { int B, N, venc, L, C[4], H[4], W[4], G; Bounds bounds; bool ties; const char* what; };

struct Problem {
    Case c; int ctot;
    std::vector<float> verts, bounds, glob, R; std::vector<float> map[4];
    std::vector<int> ext;            // per sample the lowest index holding zmin, zmax, ymin, ymax
};

// float64 restatement: rows x [B N, ctot] and, per (vertex, level), corners and weights
struct Corner { int pix[4]; double w[4]; };
static void plain_rows(const Problem& p, const std::vector<double>& v, std::vector<double>& x, std::vector<Corner>* corners) {
    const Case& c = p.c;
    x.assign((size_t)c.B * c.N * p.ctot, 0.0);
    if (corners) corners->assign((size_t)c.B * c.N * (c.L ? c.L : 1), Corner{{-1, -1, -1, -1}, {0, 0, 0, 0}});
    for (int b = 0; b < c.B; ++b) {
        const double* vb = &v[(size_t)b * c.N * 3];
        const double zmin = vb[p.ext[b * 4] * 3 + 2], zmax = vb[p.ext[b * 4 + 1] * 3 + 2], ymin = vb[p.ext[b * 4 + 2] * 3 + 1], ymax = vb[p.ext[b * 4 + 3] * 3 + 1];
        for (int i = 0; i < c.N; ++i) {
            const double* q = vb + i * 3;
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
    double s = 0;
    for (size_t i = 0; i < x.size(); ++i) s += x[i] * (double)p.R[i];
    return s;
}

static double cmp(const float* got, const std::vector<double>& want) {
    double m = 1e-30, d = 0;
    for (size_t i = 0; i < want.size(); ++i) { m = std::max(m, fabs(want[i])); d = std::max(d, fabs(want[i] - (double)got[i])); }
    return d / m;
}

static const double TOL = 2e-5;            // fp32 against float64

static int run(const Case& c) {
    Problem p; p.c = c; p.ctot = c.venc + c.G;
    for (int l = 0; l < c.L; ++l) p.ctot += c.C[l];
    const size_t rows = (size_t)c.B * c.N;
    p.verts.resize(rows * 3); p.bounds.resize((size_t)c.B * 4); p.glob.resize((size_t)c.B * c.G); p.R.resize(rows * p.ctot);
    for (float& f : p.verts) f = uni();
    if (c.ties)                               // every fifth vertex from 2 on shares zmax, from 3 on ymin; 7 holds zmax and ymax; zmin tied at 1 and 6
        for (int b = 0; b < c.B; ++b) {
            float* v = &p.verts[(size_t)b * c.N * 3];
            for (int i = 2; i < c.N; i += 5) v[i * 3 + 2] = 0.625f;
            for (int i = 3; i < c.N; i += 5) v[i * 3 + 1] = -0.625f;
            v[7 * 3 + 1] = 0.625f; v[9 * 3 + 1] = 0.625f;
            v[1 * 3 + 2] = -0.625f; v[6 * 3 + 2] = -0.625f;
        }
    for (int b = 0; b < c.B; ++b) {
        const float in[4] = {-0.8f, 0.7f, -0.6f, 0.9f}, out[4] = {-1.3f, 1.2f, -0.9f, 1.4f}, empty[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
        for (int k = 0; k < 4; ++k)
            p.bounds[b * 4 + k] = c.bounds == EMPTY_IMAGE ? empty[k] : (c.bounds == WIDE ? out[k] : in[k]) + 0.01f * b;
    }
    for (float& f : p.glob) f = rnd();
    for (float& f : p.R) f = rnd();
    for (int l = 0; l < c.L; ++l) { p.map[l].resize((size_t)c.B * c.C[l] * c.H[l] * c.W[l]); for (float& f : p.map[l]) f = rnd(); }
    p.ext.assign((size_t)c.B * 4, 0);
    for (int b = 0; b < c.B; ++b)
        for (int i = 1; i < c.N; ++i) {
            const float* v = &p.verts[(size_t)b * c.N * 3];
            int* e = &p.ext[b * 4];
            if (v[i * 3 + 2] < v[e[0] * 3 + 2]) e[0] = i;
            if (v[i * 3 + 2] > v[e[1] * 3 + 2]) e[1] = i;
            if (v[i * 3 + 1] < v[e[2] * 3 + 1]) e[2] = i;
            if (v[i * 3 + 1] > v[e[3] * 3 + 1]) e[3] = i;
        }
    int d[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = 0; l < c.L; ++l) { d[3 * l] = c.C[l]; d[3 * l + 1] = c.H[l]; d[3 * l + 2] = c.W[l]; }
#define DIMS d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]
    size_t msize = 0;
    for (int l = 0; l < c.L; ++l) msize += p.map[l].size() / c.B;
    const size_t mbytes = vpn_gcn_maps_workspace(c.B, c.L, DIMS);
    if (mbytes != (size_t)c.B * msize * 4) { puts("  maps workspace size"); return 1; }
    float *verts = al(p.verts), *bounds = al(p.bounds), *glob = c.G ? al(p.glob) : nullptr, *R = al(p.R), *f[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < c.L; ++l) f[l] = al(p.map[l]);
    float *ext = al((size_t)c.B * 4), *grid = al(rows * 2), *x = al(rows * p.ctot); int32_t* ext_idx = (int32_t*)al((size_t)c.B * 4);
    void* mws = malloc(mbytes ? mbytes : 1);
    int rc = c.L ? vpn_gcn_input_fwd(verts, bounds, glob, c.B, c.N, c.G, c.venc, c.L, f[0], f[1], f[2], f[3], DIMS, ext, ext_idx, grid, mws, x, nullptr)
                 : vpn_gcn_input_fwd(verts, nullptr, glob, c.B, c.N, c.G, c.venc, 0, nullptr, nullptr, nullptr, nullptr, DIMS, nullptr, nullptr, nullptr, nullptr, x, nullptr);
    if (rc) { printf("  fwd rc %d\n", rc); return 1; }
    int bad = 0;
    for (int b = 0; b < c.B && c.L; ++b)
        for (int k = 0; k < 4; ++k)
            if (ext_idx[b * 4 + k] != p.ext[b * 4 + k]) { printf("  sample %d extent %d: vertex %d, lowest index is %d\n", b, k, ext_idx[b * 4 + k], p.ext[b * 4 + k]); ++bad; }
    // ---- float64
    std::vector<double> v64(p.verts.begin(), p.verts.end()), x64; std::vector<Corner> corners;
    plain_rows(p, v64, x64, &corners);
    double worst = 0; const char* where = "";
    auto note = [&](const char* name, double e) { if (e > TOL) printf("  %s: rel err %.2e\n", name, e); if (e > worst) { worst = e; where = name; } };
    note("rows", cmp(x, x64));
    std::vector<double> dM[4], dG((size_t)c.B * c.G, 0.0);
    size_t outside = 0;
    for (int l = 0; l < c.L; ++l) dM[l].assign(p.map[l].size(), 0.0);
    for (size_t r = 0; r < rows; ++r) {
        int col = c.venc;
        for (int l = 0; l < c.L; ++l) {
            const Corner& cr = corners[r * c.L + l];
            const size_t hw = (size_t)c.H[l] * c.W[l];
            for (int k = 0; k < 4; ++k) {
                if (cr.pix[k] < 0) { ++outside; continue; }
                for (int ch = 0; ch < c.C[l]; ++ch) dM[l][((r / c.N) * c.C[l] + ch) * hw + cr.pix[k]] += cr.w[k] * (double)p.R[r * p.ctot + col + ch];
            }
            col += c.C[l];
        }
        for (int k = 0; k < c.G; ++k) dG[(r / c.N) * c.G + k] += (double)p.R[r * p.ctot + col + k];
    }
    // ---- backward: everything wanted, then grad_verts alone, then the map gradients alone
    const size_t wsb = vpn_gcn_input_bwd_workspace(c.B, c.N, c.L, DIMS);
    size_t cells = 0;
    for (int l = 0; l < c.L; ++l) cells += (size_t)(c.H[l] + 1) * (c.W[l] + 1) + 2;
    if (wsb != ((size_t)c.B * c.L * c.N * 4 + (size_t)c.B * cells + rows * 2 + (size_t)c.B * msize) * 4) { puts("  bwd workspace size"); return 1; }
    void* ws = malloc(wsb ? wsb : 1);
    float *gv = al(rows * 3), *gf[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; l < c.L; ++l) gf[l] = al(p.map[l].size());
    rc = vpn_gcn_input_bwd(R, verts, c.L ? bounds : nullptr, c.B, c.N, c.G, c.venc, c.L, DIMS, ext, ext_idx, grid, mws, ws, gv, gf[0], gf[1], gf[2], gf[3], nullptr);
    if (rc) { printf("  bwd rc %d\n", rc); return 1; }
    for (int l = 0; l < c.L; ++l) note("map gradient", cmp(gf[l], dM[l]));
    {
        std::vector<double> dV(rows * 3);
        const double eps = 1e-6;
        for (size_t i = 0; i < rows * 3; ++i) {
            std::vector<double> a(v64), b(v64); a[i] += eps; b[i] -= eps;
            dV[i] = (plain_loss(p, a) - plain_loss(p, b)) / (2 * eps);
        }
        note("grad_verts", cmp(gv, dV));
    }
    for (int only = 0; only < 2; ++only) {
        float *gv2 = al(rows * 3), *g2[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int l = 0; l < c.L; ++l) g2[l] = al(p.map[l].size());
        const bool m = only == 1;
        rc = vpn_gcn_input_bwd(R, verts, c.L ? bounds : nullptr, c.B, c.N, c.G, c.venc, c.L, DIMS, ext, ext_idx, grid, mws, ws, m ? nullptr : gv2,
                               m ? g2[0] : nullptr, m ? g2[1] : nullptr, m ? g2[2] : nullptr, m ? g2[3] : nullptr, nullptr);
        bool same = rc == 0 && (m || !memcmp(gv, gv2, rows * 12));
        for (int l = 0; l < c.L && m; ++l) same = same && !memcmp(gf[l], g2[l], p.map[l].size() * 4);
        if (!same) { printf("  %s alone: rc %d or another result\n", m ? "the map gradients" : "grad_verts", rc); ++bad; }
    }
    if (c.G) {     // the global block's gradient as ops.py takes it: the column sum of grad's last G columns per sample
        const size_t cb = vpn_gcn_colsum_workspace(c.B, c.N, c.G);
        if (cb != (size_t)c.B * ((c.N + 63) / 64) * c.G * 4) { puts("  colsum workspace size"); return 1; }
        void* cws = malloc(cb); float* gg = al((size_t)c.B * c.G);
        rc = vpn_gcn_colsum(R, nullptr, c.B, c.N, p.ctot, p.ctot - c.G, c.G, cws, gg, nullptr);
        if (rc) { printf("  colsum rc %d\n", rc); return 1; }
        note("global gradient", cmp(gg, dG));
    }
    size_t all = rows * 4 * (c.L ? c.L : 1);
    printf("B %d N %3d venc %2d L %d G %d  %-62s corners outside %4.1f%%  worst rel err %.2e (%s)  %s\n", c.B, c.N, c.venc, c.L, c.G, c.what,
           c.L ? 100.0 * outside / all : 0.0, worst, where, bad || worst > TOL ? "FAILED" : "ok");
    if (c.bounds == WIDE && (outside * 10 < all || outside * 10 > all * 9)) { puts("  the wide bounds leave too few corners inside or outside"); ++bad; }
    return bad || worst > TOL;
#undef DIMS
}

// vpn_gcn_aggregate over a ring of six vertices and a seventh in no edge (its self loop alone, weight 1), forward form (bias,
// ReLU) and backward form (mask), against float64
static int aggregate(int C) {
    const int B = 2, N = 7;
    std::vector<int32_t> rp(N + 1, 0), col; std::vector<float> w;
    for (int i = 0; i < 6; ++i) {
        int nb[3] = {(i + 5) % 6, i, (i + 1) % 6}; std::sort(nb, nb + 3);
        for (int k = 0; k < 3; ++k) { col.push_back(nb[k]); w.push_back(1.0f / 3.0f); }
        rp[i + 1] = (int)col.size();
    }
    col.push_back(6); w.push_back(1.0f); rp[7] = (int)col.size();
    const size_t n = (size_t)B * N * C;
    std::vector<float> x(n), bias(C), mask(n);
    for (float& f : x) f = rnd();
    for (float& f : bias) f = rnd();
    for (float& f : mask) f = rnd();
    int32_t *drp = (int32_t*)al(rp.size()), *dcol = (int32_t*)al(col.size());
    memcpy(drp, rp.data(), rp.size() * 4); memcpy(dcol, col.data(), col.size() * 4);
    float *dx = al(x), *dw = al(w), *db = al(bias), *dm = al(mask), *out = al(n);
    double worst = 0;
    for (int form = 0; form < 2; ++form) {
        const int rc = form ? vpn_gcn_aggregate(dx, drp, dcol, dw, nullptr, dm, B, N, C, 0, out, nullptr)
                            : vpn_gcn_aggregate(dx, drp, dcol, dw, db, nullptr, B, N, C, 1, out, nullptr);
        if (rc) { printf("  aggregate rc %d\n", rc); return 1; }
        std::vector<double> want(n);
        for (int b = 0; b < B; ++b) for (int i = 0; i < N; ++i) for (int ch = 0; ch < C; ++ch) {
            double s = 0;
            for (int e = rp[i]; e < rp[i + 1]; ++e) {
                const size_t src = ((size_t)b * N + col[e]) * C + ch;
                if (!form || mask[src] > 0) s += (double)w[e] * (double)x[src];
            }
            if (!form) s = std::max(s + (double)bias[ch], 0.0);
            want[((size_t)b * N + i) * C + ch] = s;
        }
        worst = std::max(worst, cmp(out, want));
    }
    char what[96];
    snprintf(what, sizeof what, "vpn_gcn_aggregate C = %d (%s), forward and backward form", C, C % 4 ? "one channel a thread" : "four channels a thread");
    printf("%-114s worst rel err %.2e  %s\n", what, worst, worst > TOL ? "FAILED" : "ok");
    return worst > TOL;
}

// vpn_gcn_colsum with R no multiple of the 64 rows of a partial sum, off > 0 and a mask
static int colsum() {
    const int S = 2, Rr = 70, ld = 9, off = 3, C = 5;
    std::vector<float> in((size_t)S * Rr * ld), mask(in.size());
    for (float& f : in) f = rnd();
    for (float& f : mask) f = rnd();
    std::vector<double> want((size_t)S * C, 0.0);
    for (int s = 0; s < S; ++s) for (int r = 0; r < Rr; ++r) for (int k = 0; k < C; ++k) {
        const size_t i = ((size_t)s * Rr + r) * ld + off + k;
        if (mask[i] > 0) want[s * C + k] += in[i];
    }
    float *din = al(in), *dm = al(mask), *out = al((size_t)S * C);
    void* ws = malloc(vpn_gcn_colsum_workspace(S, Rr, C));
    const int rc = vpn_gcn_colsum(din, dm, S, Rr, ld, off, C, ws, out, nullptr);
    const double e = rc ? 1.0 : cmp(out, want);
    printf("%-114s worst rel err %.2e  %s\n", "vpn_gcn_colsum R = 70, ld = 9, off = 3, masked", e, e > TOL ? "FAILED" : "ok");
    return e > TOL;
}

// vpn_gcn_bounds against the reference's rule read literally; exact
static int bounds_check() {
    const int B = 4, C = 2, H = 5, W = 7;
    std::vector<float> img((size_t)B * C * H * W, 0.0f);
    auto px = [&](int b, int ch, int y, int x) -> float& { return img[(((size_t)b * C + ch) * H + y) * W + x]; };
    for (int y = 1; y < 4; ++y) for (int x = 2; x < 6; ++x) { px(1, 0, y, x) = 0.02f; px(1, 1, y, x) = 0.02f; }      // image 0 stays empty
    for (int y = 0; y < H; ++y) px(2, 0, y, 0) = 0.5f;                                                              // column 0 only
    px(3, 1, H - 1, W - 1) = 0.04f; px(3, 0, 0, 3) = 0.02f;                                                          // one lit pixel, one below 0.03
    std::vector<float> want((size_t)B * 4);
    for (int b = 0; b < B; ++b) {
        int lo[2] = {0, 0}, hi[2] = {W, H}; bool any_hi[2] = {false, false};
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            float m = px(b, 0, y, x); for (int ch = 1; ch < C; ++ch) m = m + px(b, ch, y, x);
            if (!(m > 0.03f)) continue;
            const int q[2] = {x, y};
            for (int a = 0; a < 2; ++a) {
                if (q[a] >= 1 && (lo[a] == 0 || q[a] < lo[a])) lo[a] = q[a];
                if (!any_hi[a] || q[a] > hi[a]) { hi[a] = q[a]; any_hi[a] = true; }
            }
        }
        want[b * 4 + 0] = (float)lo[0] / (float)W * 2.0f - 1.0f; want[b * 4 + 1] = (float)hi[0] / (float)W * 2.0f - 1.0f;
        want[b * 4 + 2] = (float)lo[1] / (float)H * 2.0f - 1.0f; want[b * 4 + 3] = (float)hi[1] / (float)H * 2.0f - 1.0f;
    }
    float *dimg = al(img), *out = al((size_t)B * 4);
    const int rc = vpn_gcn_bounds(dimg, B, C, H, W, out, nullptr);
    const bool ok = rc == 0 && !memcmp(out, want.data(), want.size() * 4) && want[0] == -1.0f && want[1] == 1.0f && want[9] == -1.0f;
    printf("%-139s %s\n", "vpn_gcn_bounds 4 images of 2 x 5 x 7: empty, a box, column 0 only, one pixel and one below 0.03 (exact)", ok ? "ok" : "FAILED");
    return !ok;
}

int main(int argc, char** argv) {          // an argument: only the cases whose description contains it
    const Case cases[] = {
        {2, 70, 39, 3, {5, 3, 2, 0}, {4, 2, 1, 0}, {6, 3, 1, 0}, 3, EMPTY_IMAGE, false, "N = 70, non-square levels down to 1 x 1, empty-image bounds"},
        {1, 130, 3, 1, {65, 0, 0, 0}, {3, 0, 0, 0}, {2, 0, 0, 0}, 0, WIDE, false, "N = 130, C = 65, corners outside the map, no global block"},
        {2, 2, 3, 2, {3, 2, 0, 0}, {2, 1, 0, 0}, {2, 2, 0, 0}, 2, INSIDE, false, "N = 2: every vertex holds two extents, the grid terms cancel"},
        {2, 30, 3, 1, {4, 0, 0, 0}, {4, 0, 0, 0}, {5, 0, 0, 0}, 0, INSIDE, true, "tied extents"},
        {2, 5, 39, 0, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, 4, INSIDE, false, "no maps: encoding and global only"},
        {1, 6, 0, 1, {2, 0, 0, 0}, {3, 0, 0, 0}, {3, 0, 0, 0}, 0, INSIDE, false, "venc = 0: pooled columns only"},
    };
    int bad = 0;
    for (const Case& c : cases) {
        if (argc > 1 && !strstr(c.what, argv[1])) continue;
        bad += run(c);
    }
    if (argc > 1) { printf(bad ? "FAILED %d\n" : "selected ok\n", bad); return bad; }
    bad += aggregate(4) + aggregate(6) + colsum() + bounds_check();
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; int32_t i4[4];
#define ONE 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0
#define TWO 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0
        const int ok = vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 0, 5, 1, v, nullptr, nullptr, nullptr, ONE, v, i4, v, v, v, nullptr) == VPN_E_BADARG &&           // venc
                       vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 0, 3, 5, v, v, v, v, ONE, v, i4, v, v, v, nullptr) == VPN_E_BADARG &&                             // L
                       vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 0, 3, 1, nullptr, nullptr, nullptr, nullptr, ONE, v, i4, v, v, v, nullptr) == VPN_E_BADARG &&     // level pointer
                       vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 0, 3, 2, v, nullptr, nullptr, nullptr, TWO, v, i4, v, v, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 2, 3, 1, v, nullptr, nullptr, nullptr, ONE, v, i4, v, v, v, nullptr) == VPN_E_BADARG &&           // G without global
                       vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, ONE, v, i4, v, v, v, nullptr) == VPN_E_BADARG &&     // an empty row
                       vpn_gcn_input_fwd(v, v, nullptr, 1, 1, 0, 3, 1, v, nullptr, nullptr, nullptr, ONE, v, i4, v, nullptr, v, nullptr) == VPN_E_BADARG &&     // maps_ws
                       vpn_gcn_input_bwd(v, v, v, 1, 1, 0, 5, 1, ONE, v, i4, v, v, v, v, v, nullptr, nullptr, nullptr, nullptr) == VPN_E_BADARG &&              // venc
                       vpn_gcn_input_bwd(v, v, v, 1, 1, 0, 3, 5, ONE, v, i4, v, v, v, v, v, v, v, v, nullptr) == VPN_E_BADARG &&                                // L
                       vpn_gcn_input_bwd(v, v, v, 1, 1, 0, 3, 2, TWO, v, i4, v, v, v, v, v, nullptr, nullptr, nullptr, nullptr) == VPN_E_BADARG &&              // all levels or none
                       vpn_gcn_input_bwd(v, v, v, 1, 1, 0, 3, 2, TWO, v, i4, v, v, v, nullptr, nullptr, v, nullptr, nullptr, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_input_bwd(v, v, v, 1, 1, 0, 3, 1, ONE, v, i4, v, v, nullptr, v, v, nullptr, nullptr, nullptr, nullptr) == VPN_E_BADARG &&        // workspace
                       vpn_gcn_input_bwd(v, v, v, 1, 8193, 0, 3, 1, ONE, v, i4, v, v, v, nullptr, v, nullptr, nullptr, nullptr, nullptr) == VPN_E_TOOBIG &&     // the sort's limit
                       vpn_gcn_input_bwd(v, v, v, 1, 8193, 0, 3, 1, ONE, v, i4, v, v, v, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 &&          // nothing wanted
                       vpn_gcn_maps_workspace(2, 2, 3, 4, 5, 2, 1, 2, 0, 0, 0, 0, 0, 0) == 2 * (60 + 4) * 4 && vpn_gcn_maps_workspace(2, 5, ONE) == 0 &&
                       vpn_gcn_input_bwd_workspace(2, 100, 1, 3, 4, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0) == (2 * 100 * 4 + 2 * (5 * 6 + 2) + 2 * 100 * 2 + 2 * 60) * 4 &&
                       vpn_gcn_aggregate(v, nullptr, i4, v, nullptr, nullptr, 1, 1, 1, 0, v, nullptr) == VPN_E_BADARG &&
                       vpn_gcn_colsum(v, nullptr, 1, 1, 3, 2, 2, v, v, nullptr) == VPN_E_BADARG &&                                                                // ld < off + C
                       vpn_gcn_bounds(v, 1, 1, 0, 1, v, nullptr) == VPN_E_BADARG;
        printf("%-139s %s\n", "argument validation and workspace sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
