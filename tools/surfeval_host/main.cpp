// Host check of the surface evaluation (csrc/surfeval.hip) without a GPU, in the manner of
// tools/pointmesh_host: the three kernels' own source is compiled as C++ against the shim of tools/fcstack_host (a launch runs
// workgroup by workgroup on std::threads, one per work-item, real barriers) and compared with a double statement of the
// definitions: the normals of both layouts with and without an affine map, the per-sample row (sums within 2 fp32 ulps, the
// threshold counts exactly), the state against a plain loop over the rows, bit for bit.  Inputs include NaN and inf distances,
// neighbour, face and vertex indices outside their range, offset tables that do not describe the arrays, N and M that are no
// multiples of 256, more samples than one staging chunk and more (class, column) items than lanes; and the argument validation.
// Every buffer has its exact size, so AddressSanitizer sees any access past an end.  It checks indexing, barriers and the
// host-side launch logic; it says nothing about speed.
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address -Itools/fcstack_host -x c++ tools/surfeval_host/main.cpp -o surfeval_host
//   ./surfeval_host
#include "hip/hip_runtime.h"
thread_local dim3 threadIdx, blockIdx; Bar g_block; Bar g_wave[16]; float g_xch[16][64]; float g_xch2[16][64];
// the two wave exchanges the shim lacks: a double and an int travel through buffers of their own
static double g_xd[16][64]; static int g_xi[16][64];
inline double __shfl_xor(double v, int o, int) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xd[w][l] = v; g_wave[w].wait(); const double r = g_xd[w][l ^ o]; g_wave[w].wait(); return r;
}
inline int __shfl_xor(int v, int o, int) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xi[w][l] = v; g_wave[w].wait(); const int r = g_xi[w][l ^ o]; g_wave[w].wait(); return r;
}
#include "../../volumetric-primitives-net_amd/csrc/surfeval.hip"
namespace vpn { void prof_begin(const char*, hipStream_t) {} void prof_end(hipStream_t) {} }
#include <chrono>
#include <cstdio>
#include <random>
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }      // the check leaks its buffers on purpose: it exits right after
static std::mt19937 rng(28);
template <class T> static T* al(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }   // exact size: the allocation ends where the data ends
template <class T> static T* alv(const std::vector<T>& v) { T* p = al<T>(v.size()); if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

static bool within_ulps(float got, double want, int ulps) {
    if (std::isnan(want)) return std::isnan(got);
    if (std::isinf(want)) return got == (float)want;
    return fabs((double)got - want) <= ulps * 1.2e-7 * fabs(want) + 1e-45;
}

// ---- normals: the definition in double on the fp32 inputs; (0,0,0) for every index out of range and every face without area
static void normal64(const float* v0, const float* v1, const float* v2, const float* m, double out[3]) {
    double c[3][3];
    const float* v[3] = {v0, v1, v2};
    for (int k = 0; k < 3; ++k) for (int r = 0; r < 3; ++r)
        c[k][r] = m ? (double)m[4 * r] * v[k][0] + (double)m[4 * r + 1] * v[k][1] + (double)m[4 * r + 2] * v[k][2] + (double)m[4 * r + 3] : (double)v[k][r];
    double e1[3], e2[3];
    for (int r = 0; r < 3; ++r) { e1[r] = c[1][r] - c[0][r]; e2[r] = c[2][r] - c[0][r]; }
    const double x = e1[1] * e2[2] - e1[2] * e2[1], y = e1[2] * e2[0] - e1[0] * e2[2], z = e1[0] * e2[1] - e1[1] * e2[0];
    const double l = sqrt(x * x + y * y + z * z);
    out[0] = l > 0 ? x / l : 0; out[1] = l > 0 ? y / l : 0; out[2] = l > 0 ? z / l : 0;
}

// meshes: S of them with nv[s] vertices on a jittered sphere and nf[s] random well-shaped faces; ragged = packed, else S = 1 and
// B copies of the vertex block
static int run_normals(const char* name, bool ragged, int S, int sets, int n, bool with_xf, bool bad_indices, bool bad_tables) {
    std::uniform_real_distribution<float> ud(-0.5f, 0.5f);
    std::vector<int> voff(1, 0), foff(1, 0);
    for (int s = 0; s < S; ++s) { voff.push_back(voff.back() + 7 + 5 * s); foff.push_back(foff.back() + 9 + 4 * s); }
    const int B = ragged ? S * sets : 3, P = ragged ? voff.back() : 12, F = ragged ? foff.back() : 20;
    std::vector<float> verts((size_t)(ragged ? 1 : B) * P * 3);
    for (float& x : verts) x = ud(rng);
    std::vector<int> faces((size_t)F * 3), fidx((size_t)B * n);
    for (int s = 0; s < (ragged ? S : 1); ++s) {
        const int nv = ragged ? voff[s + 1] - voff[s] : P, f0 = ragged ? foff[s] : 0, f1 = ragged ? foff[s + 1] : F;
        for (int f = f0; f < f1; ++f) { const int a = rng() % nv; faces[f * 3] = a; faces[f * 3 + 1] = (a + 1 + rng() % 2) % nv; faces[f * 3 + 2] = (a + 3 + rng() % 3) % nv; }
    }
    for (int b = 0; b < B; ++b) {
        const int nf = ragged ? foff[b / sets + 1] - foff[b / sets] : F;
        for (int i = 0; i < n; ++i) fidx[(size_t)b * n + i] = rng() % nf;
    }
    if (bad_indices) {      // a face index below and above its range, a vertex index below and above its mesh, a repeated vertex
        fidx[0] = -1; fidx[1] = ragged ? foff[1] - foff[0] : F; fidx[n - 1] = 0x7fffffff; fidx[(size_t)(B - 1) * n + n - 1] = (int)0x80000000;
        faces[(size_t)fidx[2] * 3 + 1] = ragged ? voff[1] - voff[0] : P; faces[(size_t)fidx[3] * 3] = -1;
        faces[(size_t)fidx[4] * 3 + 2] = faces[(size_t)fidx[4] * 3];
    }
    if (bad_tables) { voff[1] = voff.back() + 5; foff[S] = foff[S] + 1; if (S > 2) { voff[2] = -3; } }
    std::vector<float> xf;
    if (with_xf) { xf.resize((size_t)B * 12); for (float& x : xf) x = 2 * ud(rng); for (int k = 0; k < 12; ++k) xf[k] = (k % 5 == 0) ? -1.0f : 0.0f; }   // sample 0: a point reflection
    float* d_v = alv(verts); int *d_f = alv(faces), *d_i = alv(fidx), *d_vo = alv(voff), *d_fo = alv(foff);
    float* d_x = with_xf ? alv(xf) : nullptr; float* out = al<float>((size_t)B * n * 3);
    const int rc = vpn_face_normals_at(d_v, d_f, ragged ? d_vo : nullptr, ragged ? d_fo : nullptr, d_i, d_x, B, n, P, F, sets, out, nullptr);
    bool ok = rc == 0;
    double worst = 0; int zeros = 0;
    for (int b = 0; b < B && ok; ++b) {
        const int s = b / sets;
        long long vb = ragged ? voff[s] : (long long)b * P, nv = ragged ? (long long)voff[s + 1] - voff[s] : P;
        long long fb = ragged ? foff[s] : 0, nf = ragged ? (long long)foff[s + 1] - foff[s] : F;
        if (ragged && (vb < 0 || nv < 0 || vb + nv > P)) nv = 0;
        if (ragged && (fb < 0 || nf < 0 || fb + nf > F)) nf = 0;
        for (int i = 0; i < n; ++i) {
            double want[3] = {0, 0, 0};
            const long long f = fidx[(size_t)b * n + i];
            if (f >= 0 && f < nf) {
                const int* fc = &faces[(size_t)(fb + f) * 3];
                if (fc[0] >= 0 && fc[0] < nv && fc[1] >= 0 && fc[1] < nv && fc[2] >= 0 && fc[2] < nv)
                    normal64(&verts[(size_t)(vb + fc[0]) * 3], &verts[(size_t)(vb + fc[1]) * 3], &verts[(size_t)(vb + fc[2]) * 3], with_xf ? &xf[(size_t)b * 12] : nullptr, want);
            }
            const float* got = out + ((size_t)b * n + i) * 3;
            zeros += want[0] == 0 && want[1] == 0 && want[2] == 0;
            for (int k = 0; k < 3; ++k) {
                if (want[0] == 0 && want[1] == 0 && want[2] == 0) ok = ok && got[k] == 0.0f;
                worst = std::max(worst, fabs(got[k] - want[k]));
            }
        }
    }
    ok = ok && worst <= 1e-4;       // random triangles are not conditioned: the tight bar is the GPU test's, on conditioned meshes
    printf("%-34s B %2d n %4d P %3d F %3d  worst %.2e  zero normals %4d  %s\n", name, B, n, P, F, worst, zeros, ok ? "ok" : "FAILED");
    for (void* p : {(void*)d_v, (void*)d_f, (void*)d_i, (void*)d_vo, (void*)d_fo, (void*)d_x, (void*)out}) free(p);
    return !ok;
}

// ---- the row and the state
struct Batch { int B, N, M; std::vector<float> d1, d2, np, ng; std::vector<int> i1, i2, cls; };
static Batch make_batch(int B, int N, int M, int C, bool normals, bool hostile) {
    Batch h{B, N, M};
    std::uniform_real_distribution<float> ud(0.0f, 1.0f); std::normal_distribution<float> nd(0, 1);
    auto dist = [&](std::vector<float>& d, size_t n) { d.resize(n); for (float& x : d) x = 0.05f * ud(rng); };
    dist(h.d1, (size_t)B * N); dist(h.d2, (size_t)B * M);
    h.i1.resize((size_t)B * N); h.i2.resize((size_t)B * M);
    for (int& j : h.i1) j = rng() % M;
    for (int& j : h.i2) j = rng() % N;
    if (normals) {
        auto unit = [&](std::vector<float>& v, size_t n) { v.resize(n * 3); for (size_t i = 0; i < n; ++i) { float a[3] = {nd(rng), nd(rng), nd(rng)}; const float l = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); for (int k = 0; k < 3; ++k) v[i * 3 + k] = a[k] / l; } };
        unit(h.np, (size_t)B * N); unit(h.ng, (size_t)B * M);
        for (int k = 0; k < 3; ++k) h.np[k] = 0.0f;                       // a zero normal adds 0
    }
    h.cls.resize(B);
    for (int& c : h.cls) c = rng() % C;
    if (hostile) {
        h.d1[0] = NAN; h.d2[M - 1] = INFINITY; if (N > 2) h.d1[2] = INFINITY; if (B > 1) h.d2[(size_t)M] = NAN;
        h.i1[0] = -5; h.i1[N - 1] = M; h.i2[0] = 0x7fffffff; h.i2[M - 1] = (int)0x80000000;
        h.cls[0] = -1; h.cls[B - 1] = C;
    }
    return h;
}

static void row64(const Batch& h, int b, const std::vector<float>& thr2, std::vector<double>& row, std::vector<long long>& counts) {
    const int T = (int)thr2.size(), N = h.N, M = h.M;
    row.assign(6 + 3 * T, 0.0); counts.assign(2 * T, 0);
    auto clampi = [](int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); };
    for (int dir = 0; dir < 2; ++dir) {
        const int n = dir ? M : N, no = dir ? N : M;
        const float* d = (dir ? h.d2.data() : h.d1.data()) + (size_t)b * n;
        const int* ix = (dir ? h.i2.data() : h.i1.data()) + (size_t)b * n;
        double s2 = 0, s1 = 0, nc = 0;
        for (int i = 0; i < n; ++i) {
            const double q = (double)d[i] * (double)d[i];      // the scan's distances are not squared
            s2 += q; s1 += d[i];
            for (int t = 0; t < T; ++t) counts[dir * T + t] += q < (double)thr2[t];
            if (!h.np.empty()) {
                const float* a = (dir ? h.ng.data() : h.np.data()) + ((size_t)b * n + i) * 3;
                const float* c = (dir ? h.np.data() : h.ng.data()) + ((size_t)b * no + clampi(ix[i], no)) * 3;
                nc += fabs((double)a[0] * c[0] + (double)a[1] * c[1] + (double)a[2] * c[2]);
            }
        }
        row[dir] = s2 / n; row[2 + dir] = s1 / n; row[4 + dir] = nc / n;
    }
    for (int t = 0; t < T; ++t) {
        const double p = (double)counts[t] / N, r = (double)counts[T + t] / M;
        row[6 + t] = p; row[6 + T + t] = r; row[6 + 2 * T + t] = p + r > 0 ? 2 * p * r / (p + r) : 0.0;
    }
}

static int run_meter(const char* name, const std::vector<std::pair<int, int>>& shapes, const std::vector<int>& sizes, int C, int T, bool normals, bool hostile) {
    const int W = 6 + 3 * T;
    std::vector<float> thr2;
    for (int t = 0; t < T; ++t) { const double tau = 0.05 * (t + 1) / (T + 1); thr2.push_back((float)(tau * tau)); }
    const size_t bytes = vpn_surfeval_state_size(C, T);
    bool ok = bytes == ((size_t)(1 + C) * W + 3 + C) * 8;
    double* state = (double*)calloc(1, bytes);
    std::vector<double> want_sums((size_t)(1 + C) * W, 0.0); std::vector<long long> want_counts(3 + C, 0);
    float* d_t = alv(thr2);
    int worst_ok = 1;
    for (size_t k = 0; k < sizes.size() && ok; ++k) {
        const int B = sizes[k], N = shapes[k % shapes.size()].first, M = shapes[k % shapes.size()].second;
        const Batch h = make_batch(B, N, M, C, normals, hostile);
        float *d1 = alv(h.d1), *d2 = alv(h.d2), *np = normals ? alv(h.np) : nullptr, *ng = normals ? alv(h.ng) : nullptr;
        int *i1 = alv(h.i1), *i2 = alv(h.i2), *cls = alv(h.cls);
        float* rows = al<float>((size_t)B * W);
        const int rc = vpn_surfeval_accumulate(d1, i1, d2, i2, np, ng, d_t, cls, B, N, M, T, C, state, rows, nullptr);
        ok = ok && rc == 0;
        std::vector<double> row; std::vector<long long> counts;
        for (int b = 0; b < B && ok; ++b) {
            row64(h, b, thr2, row, counts);
            for (int c = 0; c < W; ++c) worst_ok &= within_ulps(rows[(size_t)b * W + c], row[c], 2);
            for (int t = 0; t < T; ++t) {       // the counts, exactly
                worst_ok &= llround((double)rows[(size_t)b * W + 6 + t] * N) == counts[t];
                worst_ok &= llround((double)rows[(size_t)b * W + 6 + T + t] * M) == counts[T + t];
            }
            // the bookkeeping: a plain loop over the rows the kernel wrote
            for (int c = 0; c < W; ++c) want_sums[c] += (double)rows[(size_t)b * W + c];
            const int cl = h.cls[b];
            if (cl >= 0 && cl < C) { for (int c = 0; c < W; ++c) want_sums[(size_t)(1 + cl) * W + c] += (double)rows[(size_t)b * W + c]; ++want_counts[3 + cl]; }
            else ++want_counts[2];
        }
        want_counts[0] += B; want_counts[1] += 1;
        for (void* p : {(void*)d1, (void*)d2, (void*)np, (void*)ng, (void*)i1, (void*)i2, (void*)cls, (void*)rows}) free(p);
    }
    ok = ok && worst_ok;
    // bit for bit; NaN rows (hostile inputs) compare as bit patterns
    const bool state_ok = !memcmp(state, want_sums.data(), want_sums.size() * 8) && !memcmp(state + want_sums.size(), want_counts.data(), want_counts.size() * 8);
    ok = ok && state_ok;
    printf("%-34s C %3d T %d batches %zu  rows %s  state %s  %s\n", name, C, T, sizes.size(), worst_ok ? "within 2 ulps, counts exact" : "OFF", state_ok ? "bit-equal" : "DIFFERS", ok ? "ok" : "FAILED");
    free(state); free(d_t);
    return !ok;
}

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    bad += run_normals("normals, batched", false, 1, 1, 257, false, false, false);
    bad += run_normals("normals, batched, mapped", false, 1, 1, 300, true, false, false);
    bad += run_normals("normals, batched, bad indices", false, 1, 1, 65, true, true, false);
    bad += run_normals("normals, ragged, 2 sets", true, 3, 2, 257, false, false, false);
    bad += run_normals("normals, ragged, mapped", true, 2, 2, 64, true, false, false);
    bad += run_normals("normals, ragged, bad indices", true, 3, 1, 130, true, true, false);
    bad += run_normals("normals, ragged, bad tables", true, 3, 2, 70, false, false, true);
    {   // exact cases: the axis-aligned right triangle, a collinear face, three equal vertices
        const std::vector<float> v = {0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 0, 0, 5, 5, 5};
        const std::vector<int> f = {0, 1, 2, 0, 1, 3, 4, 4, 4, 1, 0, 2}, idx = {0, 1, 2, 3};
        float* d_v = alv(v); int *d_f = alv(f), *d_i = alv(idx); float* out = al<float>(12);
        bool ok = vpn_face_normals_at(d_v, d_f, nullptr, nullptr, d_i, nullptr, 1, 4, 5, 4, 1, out, nullptr) == 0;
        const float want[12] = {0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, -1};
        ok = ok && !memcmp(out, want, 32) && out[8] == 0.0f && out[11] == -1.0f && out[9] == 0.0f && out[10] == 0.0f;
        printf("%-99s %s\n", "exact normals: (0,0,1), collinear and coincident faces (0,0,0), the other winding (0,0,-1)", ok ? "ok" : "FAILED"); bad += !ok;
        free(d_v); free(d_f); free(d_i); free(out);
    }
    bad += run_meter("meter (3,257,300,3) sizes 3 3 2", {{257, 300}}, {3, 3, 2}, 5, 3, true, false);
    bad += run_meter("meter without normals", {{257, 300}, {64, 511}}, {3, 2}, 5, 2, false, false);
    bad += run_meter("meter (1,1,1,1)", {{1, 1}}, {1}, 1, 1, true, false);
    bad += run_meter("meter (2,256,64,8)", {{256, 64}}, {2}, 4, 8, true, false);
    bad += run_meter("meter, NaN / inf / bad indices", {{257, 300}, {3, 5}}, {3, 2}, 5, 3, true, true);
    bad += run_meter("meter, 300 samples, 40 classes", {{5, 3}}, {300, 7}, 40, 1, false, true);
    {   // validation without a launch
        float v[4] = {0, 0, 0, 0}; int32_t i4[4] = {0, 0, 0, 0}; double st[64];
        const int big = VPN_SURFEVAL_MAX_ITEMS + 1;
        auto nrm = [&](const void* a, const void* b, const void* vo, const void* fo, const void* c, void* o, int B, int n, int P, int F, int sets) {
            return vpn_face_normals_at((const float*)a, (const int32_t*)b, (const int32_t*)vo, (const int32_t*)fo, (const int32_t*)c, nullptr, B, n, P, F, sets, (float*)o, nullptr); };
        bool ok = nrm(nullptr, i4, nullptr, nullptr, i4, v, 1, 1, 1, 1, 1) == VPN_E_BADARG && nrm(v, nullptr, nullptr, nullptr, i4, v, 1, 1, 1, 1, 1) == VPN_E_BADARG &&
                  nrm(v, i4, nullptr, nullptr, nullptr, v, 1, 1, 1, 1, 1) == VPN_E_BADARG && nrm(v, i4, nullptr, nullptr, i4, nullptr, 1, 1, 1, 1, 1) == VPN_E_BADARG &&
                  nrm(v, i4, i4, nullptr, i4, v, 1, 1, 1, 1, 1) == VPN_E_BADARG && nrm(v, i4, nullptr, i4, i4, v, 1, 1, 1, 1, 1) == VPN_E_BADARG &&
                  nrm(v, i4, i4, i4, i4, v, 3, 1, 1, 1, 2) == VPN_E_BADARG;
        for (int k = 0; k < 5; ++k) { int a[5] = {1, 1, 1, 1, 1}; a[k] = 0; ok = ok && nrm(v, i4, nullptr, nullptr, i4, v, a[0], a[1], a[2], a[3], a[4]) == VPN_E_BADARG; }
        ok = ok && nrm(v, i4, nullptr, nullptr, i4, v, 65536, 1, 1, 1, 1) == VPN_E_TOOBIG && nrm(v, i4, nullptr, nullptr, i4, v, 1, big, 1, 1, 1) == VPN_E_TOOBIG &&
             nrm(v, i4, nullptr, nullptr, i4, v, 1, 1, big, 1, 1) == VPN_E_TOOBIG && nrm(v, i4, nullptr, nullptr, i4, v, 1, 1, 1, big, 1) == VPN_E_TOOBIG;
        auto acc = [&](int null_at, const float* np, const float* ng, int B, int N, int M, int T, int C, void* state) {
            const void* p[8] = {v, i4, v, i4, v, i4, state, v}; if (null_at >= 0) p[null_at] = nullptr;
            return vpn_surfeval_accumulate((const float*)p[0], (const int32_t*)p[1], (const float*)p[2], (const int32_t*)p[3], np, ng, (const float*)p[4], (const int32_t*)p[5],
                                           B, N, M, T, C, (void*)p[6], (float*)p[7], nullptr); };
        for (int k = 0; k < 8; ++k) ok = ok && acc(k, nullptr, nullptr, 1, 1, 1, 1, 1, st) == VPN_E_BADARG;
        ok = ok && acc(-1, v, nullptr, 1, 1, 1, 1, 1, st) == VPN_E_BADARG && acc(-1, nullptr, v, 1, 1, 1, 1, 1, st) == VPN_E_BADARG &&
             acc(-1, nullptr, nullptr, 1, 1, 1, 1, 1, (char*)st + 4) == VPN_E_BADARG;
        for (int k = 0; k < 5; ++k) { int a[5] = {1, 1, 1, 1, 1}; a[k] = 0; ok = ok && acc(-1, nullptr, nullptr, a[0], a[1], a[2], a[3], a[4], st) == VPN_E_BADARG; }
        ok = ok && acc(-1, nullptr, nullptr, 65536, 1, 1, 1, 1, st) == VPN_E_TOOBIG && acc(-1, nullptr, nullptr, 1, big, 1, 1, 1, st) == VPN_E_TOOBIG &&
             acc(-1, nullptr, nullptr, 1, 1, big, 1, 1, st) == VPN_E_TOOBIG && acc(-1, nullptr, nullptr, 1, 1, 1, 9, 1, st) == VPN_E_TOOBIG &&
             acc(-1, nullptr, nullptr, 1, 1, 1, 1, big, st) == VPN_E_TOOBIG;
        ok = ok && vpn_surfeval_state_size(13, 2) == (14 * 12 + 16) * 8 && vpn_surfeval_state_size(0, 2) == 0 && vpn_surfeval_state_size(1, 0) == 0 &&
             vpn_surfeval_state_size(1, 9) == 0 && vpn_surfeval_state_size(big, 1) == 0;
        printf("%-99s %s\n", "argument validation and state sizes", ok ? "ok" : "FAILED"); bad += !ok;
    }
    printf("%.0f s of wall time\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf(bad ? "FAILED %d\n" : "all ok\n", bad); return bad;
}
