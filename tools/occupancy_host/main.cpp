// Host check of the volumetric evaluation (csrc/occupancy.hip) without a GPU, in the manner of
// tools/surfeval_host: the six kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers) and compared with a double statement of the
// definitions: the occupancy and owner of a primitive assembly, the winding number of both layouts with and without an affine
// map, the integer counts and the row of the IoU, the state against a plain loop over the rows, bit for bit.  Inputs include NaN
// and inf coordinates, vertex indices outside their mesh, faces of no area, offset tables that do not describe the arrays, Q and F
// that are no multiples of the tile and the slice, more primitives than one staging, more samples than one staging chunk and more
// (class, column) items than lanes; and every rejected argument.  Every buffer has its exact size, so AddressSanitizer sees any
// access past an end.  It checks indexing, barriers and the host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/occupancy_host/main.cpp -o occupancy_host
//   ./occupancy_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
// the wave exchange the shim lacks: an int travels through a buffer of its own
static int g_xi[16][64];
inline int __shfl_xor(int v, int o, int) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xi[w][l] = v; g_wave[w].wait(); const int r = g_xi[w][l ^ o]; g_wave[w].wait(); return r;
}
#include "../../volumetric-primitives-net_amd/csrc/occupancy.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <chrono>
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(29);
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
template <class T> static T* alv(const std::vector<T>& v) { T* p = al<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }
static void* al16(size_t bytes) { void* p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 16)) return nullptr; return p; }   // exact size, 16-byte aligned

// ---- primitives: the definition in double on the fp32 inputs
static void rotation64(const float* q, double R[3][3]) {
    const double PI32 = 3.1415927410125732;
    const double r = (double)q[3] - floor((double)q[3]), h = ((r * 2) * PI32) / 2;
    const double a = q[0] * sin(h), b = q[1] * sin(h), c = q[2] * sin(h), d = cos(h), l = sqrt(a * a + b * b + c * c + d * d);
    const double x = a / l, y = b / l, z = c / l, w = d / l;
    R[0][0] = x * x - y * y - z * z + w * w; R[0][1] = 2 * (x * y - z * w); R[0][2] = 2 * (x * z + y * w);
    R[1][0] = 2 * (x * y + z * w); R[1][1] = -x * x + y * y - z * z + w * w; R[1][2] = 2 * (y * z - x * w);
    R[2][0] = 2 * (x * z - y * w); R[2][1] = 2 * (y * z + x * w); R[2][2] = -x * x - y * y + z * z + w * w;
}
static double prim_m64(const float* prm, int kind, const float* x) {
    double R[3][3]; rotation64(prm + 3, R);
    const double d[3] = {(double)x[0] - prm[7], (double)x[1] - prm[8], (double)x[2] - prm[9]};
    double y[3];
    for (int i = 0; i < 3; ++i) y[i] = (R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2]) / prm[i];
    if (std::isnan(y[0]) || std::isnan(y[1]) || std::isnan(y[2])) return NAN;
    return kind == VPN_SPHERE ? y[0] * y[0] + y[1] * y[1] + y[2] * y[2] : std::max(fabs(y[0]), std::max(fabs(y[1]), fabs(y[2])));
}

static int run_prims(const char* name, int B, int K, int Q, bool shared, bool hostile) {
    std::uniform_real_distribution<float> ud(-0.5f, 0.5f), uv(0.1f, 0.4f);
    std::vector<float> params((size_t)B * K * 10), q((size_t)(shared ? 1 : B) * Q * 3);
    std::vector<int> kinds(K);
    for (int i = 0; i < B * K; ++i) { float* p = &params[(size_t)i * 10]; for (int k = 0; k < 3; ++k) p[k] = uv(rng); for (int k = 3; k < 7; ++k) p[k] = 2 * ud(rng); for (int k = 7; k < 10; ++k) p[k] = 0.6f * ud(rng); }
    for (int& k : kinds) k = rng() % 2;
    for (float& x : q) x = 1.2f * ud(rng);
    if (hostile) { q[0] = NAN; q[4] = INFINITY; params[0] = 0.0f; params[10 + 1] = NAN; params[(size_t)(B * K - 1) * 10 + 3] = INFINITY; if (K > 2) kinds[2] = 7; }
    float *d_p = alv(params), *d_q = alv(q); int* d_k = alv(kinds);
    uint8_t* occ = al<uint8_t>((size_t)B * Q); int32_t* owner = al<int32_t>((size_t)B * Q);
    bool ok = vpn_occupancy_prims(d_p, d_k, d_q, shared, B, K, Q, occ, owner, nullptr) == 0;
    ok = ok && vpn_occupancy_prims(d_p, d_k, d_q, shared, B, K, Q, occ, nullptr, nullptr) == 0 && vpn_occupancy_prims(d_p, d_k, d_q, shared, B, K, Q, nullptr, owner, nullptr) == 0;
    int near = 0, wrong = 0, inside = 0;
    for (int b = 0; b < B && ok; ++b) for (int i = 0; i < Q; ++i) {
        const float* x = &q[((size_t)(shared ? 0 : b) * Q + i) * 3];
        int want = -1; bool unsure = false;
        for (int k = 0; k < K; ++k) {
            const double m = prim_m64(&params[((size_t)b * K + k) * 10], kinds[k] == VPN_SPHERE ? VPN_SPHERE : VPN_CUBOID, x);
            if (fabs(m - 1) < 1e-4) { unsure = true; break; }              // the decision is the GPU test's, on conditioned inputs
            if (m <= 1) { want = k; break; }
        }
        const size_t o = (size_t)b * Q + i;
        if (unsure) { ++near; continue; }
        wrong += owner[o] != want || occ[o] != (want >= 0);
        inside += want >= 0;
    }
    ok = ok && wrong == 0 && near <= B * Q / 50;
    printf("%-34s B %2d K %3d Q %4d  inside %5d  within 1e-4 of a boundary %3d  wrong %d  %s\n", name, B, K, Q, inside, near, wrong, ok ? "ok" : "FAILED");
    free(d_p); free(d_q); free(d_k); free(occ); free(owner);
    return !ok;
}

// ---- the winding number: the definition in double on the fp32 inputs
static double winding64(const std::vector<float>& verts, long long vbase, long long nv, const std::vector<int>& faces, long long fbase, long long nf,
                        const float* m, const float* x) {
    double total = 0; bool bad = !(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]));
    for (long long f = 0; f < nf; ++f) {
        const int* fc = &faces[(size_t)(fbase + f) * 3];
        if (!(fc[0] >= 0 && fc[0] < nv && fc[1] >= 0 && fc[1] < nv && fc[2] >= 0 && fc[2] < nv)) continue;
        float cf[3][3]; double c[3][3]; bool fin = true;
        for (int k = 0; k < 3; ++k) {
            const float* v = &verts[(size_t)(vbase + fc[k]) * 3];
            for (int r = 0; r < 3; ++r) { cf[k][r] = m ? m[4 * r] * v[0] + m[4 * r + 1] * v[1] + m[4 * r + 2] * v[2] + m[4 * r + 3] : v[r]; c[k][r] = cf[k][r]; fin = fin && std::isfinite(cf[k][r]); }
        }
        if (!fin) { bad = true; continue; }
        const float e1[3] = {cf[1][0] - cf[0][0], cf[1][1] - cf[0][1], cf[1][2] - cf[0][2]}, e2[3] = {cf[2][0] - cf[0][0], cf[2][1] - cf[0][1], cf[2][2] - cf[0][2]};
        if (e1[1] * e2[2] - e1[2] * e2[1] == 0 && e1[2] * e2[0] - e1[0] * e2[2] == 0 && e1[0] * e2[1] - e1[1] * e2[0] == 0) continue;   // no area: the kernel's own fp32 test on the mapped fp32 corners
        double a[3], b[3], d[3];
        for (int r = 0; r < 3; ++r) { a[r] = c[0][r] - x[r]; b[r] = c[1][r] - x[r]; d[r] = c[2][r] - x[r]; }
        auto dot = [](const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; };
        const double la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), lc = sqrt(dot(d, d));
        const double n[3] = {b[1] * d[2] - b[2] * d[1], b[2] * d[0] - b[0] * d[2], b[0] * d[1] - b[1] * d[0]};
        const double num = dot(a, n), den = la * lb * lc + dot(a, b) * lc + dot(b, d) * la + dot(d, a) * lb;
        total += num == 0 ? 0.0 : 2 * atan2(num, den);
    }
    return bad ? NAN : total / (4 * M_PI);
}

// S closed meshes of different sizes: `rings` rings of `seg` vertices on an ellipsoid and two poles, rings * seg + 2 vertices and
// 2 seg rings outward faces, every one well shaped; ragged = packed (mesh s has rings + 2 s rings), else the first mesh with B
// jittered copies of its vertices
static int run_winding(const char* name, bool ragged, int B, int seg, int rings0, int Q, bool shared, bool with_xf, bool hostile, bool bad_tables, int plan_faces) {
    std::uniform_real_distribution<float> ud(-0.5f, 0.5f);
    const int S = ragged ? B : 1;
    std::vector<int> voff(1, 0), foff(1, 0), faces;
    std::vector<float> verts;
    auto add_mesh = [&](int rings, float jitter) {
        const float cx = 0.1f * ud(rng), cy = 0.1f * ud(rng), cz = 0.1f * ud(rng);
        for (int r = 0; r < rings; ++r) for (int i = 0; i < seg; ++i) {
            const float th = 3.14159265f * (r + 1) / (rings + 1), t = 6.2831853f * i / seg;
            verts.insert(verts.end(), {cx + 0.3f * sinf(th) * cosf(t) + jitter * ud(rng), cy + 0.3f * sinf(th) * sinf(t) + jitter * ud(rng), cz + 0.35f * cosf(th) + jitter * ud(rng)});
        }
        verts.insert(verts.end(), {cx, cy, cz + 0.35f, cx, cy, cz - 0.35f});
    };
    for (int s = 0; s < S; ++s) {
        const int rings = rings0 + 2 * s, top = rings * seg, bottom = top + 1;
        for (int i = 0; i < seg; ++i) {
            const int j = (i + 1) % seg;
            faces.insert(faces.end(), {i, j, top}); faces.insert(faces.end(), {(rings - 1) * seg + j, (rings - 1) * seg + i, bottom});
            for (int r = 0; r + 1 < rings; ++r) { faces.insert(faces.end(), {r * seg + i, (r + 1) * seg + i, (r + 1) * seg + j}); faces.insert(faces.end(), {r * seg + i, (r + 1) * seg + j, r * seg + j}); }
        }
        voff.push_back(voff.back() + rings * seg + 2); foff.push_back(foff.back() + 2 * seg * rings);
        if (ragged) add_mesh(rings, 0.004f);
    }
    const int P = ragged ? voff.back() : rings0 * seg + 2, F = foff.back();
    if (!ragged) for (int b = 0; b < B; ++b) add_mesh(rings0, 0.004f);
    if (hostile) {      // indices below and above the mesh, faces of no area, a corner that is not finite in the LAST sample only
        faces[3 * 1] = -1; faces[3 * 2 + 1] = ragged ? voff[1] : P; faces[3 * 3 + 2] = 0x7fffffff; faces[3 * 4] = (int)0x80000000;
        faces[3 * 5 + 1] = faces[3 * 5]; faces[3 * 6 + 2] = faces[3 * 6 + 1];
        verts[((size_t)(ragged ? voff[S - 1] : (size_t)(B - 1) * P) + 3) * 3 + 1] = INFINITY;
    }
    std::vector<float> q((size_t)(shared ? 1 : B) * Q * 3);
    for (float& x : q) x = 1.2f * ud(rng);
    if (hostile) { q[0] = NAN; q[5] = -INFINITY; for (int k = 0; k < 3; ++k) q[6 + k] = verts[k]; }      // and a query ON a vertex
    std::vector<int> true_foff = foff, true_voff = voff;
    if (bad_tables) { foff[S] = foff[S] + 1; voff[1] = voff.back() + 5; if (S > 2) foff[1] = -3; }
    std::vector<float> xf;
    if (with_xf) { xf.resize((size_t)B * 12); for (float& x : xf) x = 2 * ud(rng); for (int k = 0; k < 12; ++k) xf[k] = (k % 5 == 0) ? -1.0f : 0.0f; }   // sample 0: a point reflection
    int max_faces = 0;
    for (int s = 0; s < S; ++s) max_faces = std::max(max_faces, true_foff[s + 1] - true_foff[s]);
    if (plan_faces) max_faces = plan_faces;
    float *d_v = alv(verts), *d_q = alv(q), *d_x = with_xf ? alv(xf) : nullptr; int *d_f = alv(faces), *d_vo = alv(voff), *d_fo = alv(foff);
    const size_t bytes = vpn_winding_workspace(B, Q, F, ragged, max_faces);
    void* ws = al16(bytes);
    float* w = al<float>((size_t)B * Q); uint8_t* occ = al<uint8_t>((size_t)B * Q);
    int sf = 0; const int slices = vpn_winding_plan(B, Q, ragged ? max_faces : F, &sf);
    bool ok = bytes > 0 && vpn_winding_number(d_v, d_f, ragged ? d_vo : nullptr, ragged ? d_fo : nullptr, d_x, d_q, shared, B, Q, P, F, max_faces, ws, bytes, w, occ, nullptr) == 0;
    double worst = 0; int nans = 0, wrong_occ = 0;
    for (int b = 0; b < B && ok; ++b) {
        long long vb = ragged ? voff[b] : (long long)b * P, nv = ragged ? (long long)voff[b + 1] - voff[b] : P;
        long long fb = ragged ? foff[b] : 0, nf = ragged ? (long long)foff[b + 1] - foff[b] : F;
        if (ragged && (vb < 0 || nv < 0 || vb + nv > P)) { vb = 0; nv = 0; }
        if (ragged && (fb < 0 || nf < 0 || fb + nf > F)) { fb = 0; nf = 0; }
        for (int i = 0; i < Q; ++i) {
            const double want = winding64(verts, vb, nv, faces, fb, nf, with_xf ? &xf[(size_t)b * 12] : nullptr, &q[((size_t)(shared ? 0 : b) * Q + i) * 3]);
            const float got = w[(size_t)b * Q + i];
            if (std::isnan(want)) { ++nans; ok = ok && std::isnan(got); } else worst = std::max(worst, fabs(got - want));
            wrong_occ += occ[(size_t)b * Q + i] != (got > 0.5f);
        }
    }
    ok = ok && worst <= 1e-4 && wrong_occ == 0;     // random queries are not conditioned: the decisions against float64 are the GPU test's
    printf("%-34s B %2d Q %4d P %4d F %4d  slices %2d x %4d  worst %.2e  NaN %4d  %s\n", name, B, Q, P, F, slices, sf, worst, nans, ok ? "ok" : "FAILED");
    for (void* p : {(void*)d_v, (void*)d_q, (void*)d_x, (void*)d_f, (void*)d_vo, (void*)d_fo, ws, (void*)w, (void*)occ}) free(p);
    return !ok;
}

// ---- the IoU row and the state
static int run_meter(const char* name, const std::vector<int>& sizes, int Q, int C, bool hostile) {
    const int W = VPN_VOLIOU_WIDTH;
    const size_t bytes = vpn_voliou_state_size(C);
    bool ok = bytes == ((size_t)(1 + C) * W + 4 + C) * 8;
    double* state = (double*)calloc(1, bytes);
    std::vector<double> want_sums((size_t)(1 + C) * W, 0.0); std::vector<long long> want_counts(4 + C, 0);
    bool rows_ok = true;
    for (size_t k = 0; k < sizes.size() && ok; ++k) {
        const int B = sizes[k];
        std::vector<uint8_t> p((size_t)B * Q), g((size_t)B * Q); std::vector<int> cls(B);
        for (auto& x : p) x = rng() % 5 < 2 ? (uint8_t)(1 + rng() % 255) : 0;
        for (auto& x : g) x = rng() % 2;
        for (int& c : cls) c = rng() % C;
        if (hostile) { cls[0] = -1; cls[B - 1] = C; for (int i = 0; i < Q; ++i) p[i] = g[i] = 0; if (B > 1) for (int i = 0; i < Q; ++i) p[(size_t)Q + i] = 0; }
        uint8_t *d_p = alv(p), *d_g = alv(g); int* d_c = alv(cls);
        float* rows = al<float>((size_t)B * W); int32_t* counts = al<int32_t>((size_t)B * 4);
        ok = ok && vpn_voliou_accumulate(d_p, d_g, d_c, B, Q, C, state, rows, counts, nullptr) == 0;
        for (int b = 0; b < B && ok; ++b) {
            long long n[4] = {0, 0, 0, 0};
            for (int i = 0; i < Q; ++i) { const int a = p[(size_t)b * Q + i] != 0, d = g[(size_t)b * Q + i] != 0; n[0] += a & d; n[1] += a | d; n[2] += a; n[3] += d; }
            for (int j = 0; j < 4; ++j) rows_ok = rows_ok && counts[b * 4 + j] == n[j];
            const long long num[5] = {n[0], n[0], n[0], n[2], n[3]}, den[5] = {n[1], n[2], n[3], Q, Q};
            for (int j = 0; j < W; ++j) rows_ok = rows_ok && rows[(size_t)b * W + j] == (den[j] ? (float)((double)num[j] / (double)den[j]) : 0.0f);
            for (int j = 0; j < W; ++j) want_sums[j] += (double)rows[(size_t)b * W + j];
            const int cl = cls[b];
            if (cl >= 0 && cl < C) { for (int j = 0; j < W; ++j) want_sums[(size_t)(1 + cl) * W + j] += (double)rows[(size_t)b * W + j]; ++want_counts[4 + cl]; }
            else ++want_counts[3];
            want_counts[2] += n[1] == 0;
        }
        want_counts[0] += B; want_counts[1] += 1;
        for (void* x : {(void*)d_p, (void*)d_g, (void*)d_c, (void*)rows, (void*)counts}) free(x);
    }
    const bool state_ok = !memcmp(state, want_sums.data(), want_sums.size() * 8) && !memcmp(state + want_sums.size(), want_counts.data(), want_counts.size() * 8);
    ok = ok && rows_ok && state_ok;
    printf("%-34s C %3d Q %4d batches %zu  rows %s  state %s  empty %lld  %s\n", name, C, Q, sizes.size(), rows_ok ? "and counts exact" : "OFF", state_ok ? "bit-equal" : "DIFFERS", want_counts[2], ok ? "ok" : "FAILED");
    free(state);
    return !ok;
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    bad += run_prims("primitives, shared queries", 2, 3, 300, true, false);
    bad += run_prims("primitives, K = 1, Q = 1", 1, 1, 1, false, false);
    bad += run_prims("primitives, two stagings", 2, 300, 257, false, false);
    bad += run_prims("primitives, NaN / inf / zero extent", 3, 5, 70, false, true);
    bad += run_winding("winding, batched, 3 slices", false, 2, 16, 10, 300, false, false, false, false, 0);
    bad += run_winding("winding, batched, shared, mapped", false, 3, 8, 3, 65, true, true, false, false, 0);
    bad += run_winding("winding, batched, hostile", false, 2, 10, 7, 130, false, true, true, false, 0);
    bad += run_winding("winding, Q = 1, F = 6", false, 1, 3, 1, 1, true, false, false, false, 0);
    bad += run_winding("winding, ragged", true, 3, 12, 4, 257, false, false, false, false, 0);
    bad += run_winding("winding, ragged, shared, mapped", true, 3, 16, 7, 100, true, true, false, false, 0);
    bad += run_winding("winding, ragged, hostile", true, 3, 16, 7, 130, false, true, true, false, 0);
    bad += run_winding("winding, ragged, bad tables", true, 3, 10, 4, 70, false, false, false, true, 0);
    bad += run_winding("winding, ragged, a short plan", true, 2, 16, 9, 64, false, false, false, false, 130);
    {   // exact cases: one face seen from a vertex and from its plane, faces of no area, indices outside the mesh
        const std::vector<float> v = {0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 0, 0, 5, 5, 5}, q = {0, 0, 0, 0.25f, 0.25f, 0, 7, -3, 0, 1, 0, 0};
        const std::vector<int> f = {0, 1, 2, 0, 1, 3, 4, 4, 4, 0, 1, 5, -1, 1, 2};
        float *d_v = alv(v), *d_q = alv(q); int* d_f = alv(f); float* w = al<float>(4);
        const size_t bytes = vpn_winding_workspace(1, 4, 5, 0, 0); void* ws = al16(bytes);
        bool ok = vpn_winding_number(d_v, d_f, nullptr, nullptr, nullptr, d_q, 1, 1, 4, 5, 5, 0, ws, bytes, w, nullptr, nullptr) == 0;
        ok = ok && w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f;
        const std::vector<float> above = {0.25f, 0.25f, -1e-3f}; float* d_a = alv(above);      // just below the face, whose normal points up: the inner side, w near +1/2
        ok = ok && vpn_winding_number(d_v, d_f, nullptr, nullptr, nullptr, d_a, 1, 1, 1, 5, 5, 0, ws, bytes, w, nullptr, nullptr) == 0 && w[0] > 0.45f && w[0] < 0.5f;
        printf("%-99s %s\n", "exact zeros: on a vertex, on the plane, no area, indices outside; the sign below an upward face", ok ? "ok" : "FAILED"); bad += !ok;
        free(d_v); free(d_q); free(d_f); free(w); free(ws); free(d_a);
    }
    bad += run_meter("meter, sizes 3 3 2", {3, 3, 2}, 769, 5, false);
    bad += run_meter("meter (1, 1, 1)", {1}, 1, 1, false);
    bad += run_meter("meter, empty unions, bad classes", {3, 2}, 300, 5, true);
    bad += run_meter("meter, 300 samples, 60 classes", {300, 7}, 70, 60, true);
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; int32_t i4[4] = {0, 0, 0, 0}; alignas(16) double st[64]; uint8_t u[4] = {0, 0, 0, 0};
        const int big = VPN_OCCUPANCY_MAX_ITEMS + 1;
        auto prm = [&](int null_at, int B, int K, int Q) { const void* p[5] = {v, i4, v, u, i4}; if (null_at >= 0) p[null_at] = nullptr; if (null_at == 3) p[4] = nullptr;
            return vpn_occupancy_prims((const float*)p[0], (const int32_t*)p[1], (const float*)p[2], 1, B, K, Q, (uint8_t*)p[3], (int32_t*)p[4], nullptr); };
        bool ok = prm(0, 1, 1, 1) == VPN_E_BADARG && prm(1, 1, 1, 1) == VPN_E_BADARG && prm(2, 1, 1, 1) == VPN_E_BADARG && prm(3, 1, 1, 1) == VPN_E_BADARG;
        ok = ok && prm(-1, 0, 1, 1) == VPN_E_BADARG && prm(-1, 1, 0, 1) == VPN_E_BADARG && prm(-1, 1, 1, 0) == VPN_E_BADARG;
        ok = ok && prm(-1, 65536, 1, 1) == VPN_E_TOOBIG && prm(-1, 1, VPN_MAX_PRIMS + 1, 1) == VPN_E_TOOBIG && prm(-1, 1, 1, big) == VPN_E_TOOBIG;
        auto wnd = [&](int null_at, const void* vo, const void* fo, int B, int Q, int P, int F, int mf, void* ws, size_t bytes) { const void* p[5] = {v, i4, v, v, u}; if (null_at >= 0) p[null_at] = nullptr; if (null_at == 3) p[4] = nullptr;
            return vpn_winding_number((const float*)p[0], (const int32_t*)p[1], (const int32_t*)vo, (const int32_t*)fo, nullptr, (const float*)p[2], 1, B, Q, P, F, mf, ws, bytes, (float*)p[3], (uint8_t*)p[4], nullptr); };
        const size_t need = vpn_winding_workspace(1, 1, 1, 0, 0);
        for (int k = 0; k < 4; ++k) ok = ok && wnd(k, nullptr, nullptr, 1, 1, 1, 1, 1, st, 512) == VPN_E_BADARG;
        ok = ok && wnd(-1, i4, nullptr, 1, 1, 1, 1, 1, st, 512) == VPN_E_BADARG && wnd(-1, nullptr, i4, 1, 1, 1, 1, 1, st, 512) == VPN_E_BADARG;
        ok = ok && wnd(-1, nullptr, nullptr, 1, 1, 1, 1, 1, nullptr, 512) == VPN_E_BADARG && wnd(-1, nullptr, nullptr, 1, 1, 1, 1, 1, st, need - 1) == VPN_E_BADARG;
        ok = ok && wnd(-1, nullptr, nullptr, 1, 1, 1, 1, 1, (char*)st + 8, 504) == VPN_E_BADARG;
        ok = ok && wnd(-1, i4, i4, 1, 1, 1, 4, 0, st, 512) == VPN_E_BADARG && wnd(-1, i4, i4, 1, 1, 1, 4, 5, st, 512) == VPN_E_BADARG;
        for (int k = 0; k < 4; ++k) { int a[4] = {1, 1, 1, 1}; a[k] = 0; ok = ok && wnd(-1, nullptr, nullptr, a[0], a[1], a[2], a[3], 1, st, 512) == VPN_E_BADARG; }
        ok = ok && wnd(-1, nullptr, nullptr, 65536, 1, 1, 1, 1, st, 512) == VPN_E_TOOBIG && wnd(-1, nullptr, nullptr, 1, big, 1, 1, 1, st, 512) == VPN_E_TOOBIG &&
             wnd(-1, nullptr, nullptr, 1, 1, big, 1, 1, st, 512) == VPN_E_TOOBIG && wnd(-1, nullptr, nullptr, 1, 1, 1, big, 1, st, 512) == VPN_E_TOOBIG;
        ok = ok && need == 16 + 48 && vpn_winding_workspace(0, 1, 1, 0, 0) == 0 && vpn_winding_workspace(1, 1, 4, 1, 5) == 0 && vpn_winding_workspace(1, big, 1, 0, 0) == 0;
        int sf = 0;
        ok = ok && vpn_winding_plan(3, 257, 320, &sf) == 3 && sf == 107 && vpn_winding_plan(1, 1, 0, &sf) == VPN_E_BADARG && vpn_winding_plan(1, 1, big, nullptr) == VPN_E_TOOBIG;
        auto acc = [&](int null_at, int B, int Q, int C, void* state) { const void* p[6] = {u, u, i4, state, v, i4}; if (null_at >= 0) p[null_at] = nullptr;
            return vpn_voliou_accumulate((const uint8_t*)p[0], (const uint8_t*)p[1], (const int32_t*)p[2], B, Q, C, (void*)p[3], (float*)p[4], (int32_t*)p[5], nullptr); };
        for (int k = 0; k < 6; ++k) ok = ok && acc(k, 1, 1, 1, st) == VPN_E_BADARG;
        ok = ok && acc(-1, 1, 1, 1, (char*)st + 4) == VPN_E_BADARG && acc(-1, 0, 1, 1, st) == VPN_E_BADARG && acc(-1, 1, 0, 1, st) == VPN_E_BADARG && acc(-1, 1, 1, 0, st) == VPN_E_BADARG;
        ok = ok && acc(-1, 65536, 1, 1, st) == VPN_E_TOOBIG && acc(-1, 1, big, 1, st) == VPN_E_TOOBIG && acc(-1, 1, 1, big, st) == VPN_E_TOOBIG;
        ok = ok && vpn_voliou_state_size(13) == (14 * 5 + 17) * 8 && vpn_voliou_state_size(0) == 0 && vpn_voliou_state_size(big) == 0;
        printf("%-99s %s\n", "argument validation, plan, workspace and state sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf("%.0f s of wall time\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
