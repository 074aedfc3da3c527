#pragma once
// host shim: runs a HIP kernel block by block on std::threads (experiment only)
#define VPN_HOST_SHIM 1
#include <cmath>
#include <type_traits>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <mutex>
#include <condition_variable>
#include <algorithm>
#define __device__
#define __global__
#define __host__
#define __restrict__
#define __launch_bounds__(...)
#define __forceinline__ inline
#define __shared__ static
typedef int hipError_t; const int hipSuccess = 0; typedef void* hipStream_t;
inline hipError_t hipGetLastError() { return 0; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float4 { float x, y, z, w; };
inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
extern thread_local dim3 threadIdx, blockIdx;
using std::min;
inline float __expf(float x) { return expf(x); }
inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
struct Bar {
    std::mutex m; std::condition_variable cv; int live = 0, waiting = 0; long gen = 0;
    void wait() { std::unique_lock<std::mutex> l(m); long g = gen; if (++waiting == live) { waiting = 0; ++gen; cv.notify_all(); } else cv.wait(l, [&] { return gen != g; }); }
    void drop() { std::unique_lock<std::mutex> l(m); --live; if (live > 0 && waiting == live) { waiting = 0; ++gen; cv.notify_all(); } }
};
extern Bar g_block; extern Bar g_wave[16]; extern float g_xch[16][64];
inline void __syncthreads() { g_block.wait(); }
inline float __shfl_xor(float v, int o, int) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = v; g_wave[w].wait(); float r = g_xch[w][l ^ o]; g_wave[w].wait(); return r;
}
// the f32-input MFMAs (tools/trunkconv_host): every lane publishes its A and B element through the per-wave exchange buffers
// (g_xch, g_xch2), then forms its own results as the k-ordered fmaf chain of the instruction.  Operand and result maps of
// gfx950: 32x32x2 A[l & 31][l >> 5], B[l >> 5][l & 31], D column l & 31, row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5);
// 16x16x4 A[l & 15][l >> 4], B[l >> 4][l & 15], D column l & 15, row 4 (l >> 4) + reg.
extern float g_xch2[16][64];
struct f32x16 { float v[16]; float& operator[](int i) { return v[i]; } const float& operator[](int i) const { return v[i]; } };
struct f32x4 { float v[4]; float& operator[](int i) { return v[i]; } const float& operator[](int i) const { return v[i]; } };
inline f32x16 __builtin_amdgcn_mfma_f32_32x32x2f32(float a, float b, f32x16 c, int, int, int) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = a; g_xch2[w][l] = b; g_wave[w].wait();
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
        for (int k = 0; k < 2; ++k) c[r] = fmaf(g_xch[w][i + 32 * k], g_xch2[w][j + 32 * k], c[r]);
    }
    g_wave[w].wait(); return c;
}
inline f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float a, float b, f32x4 c, int, int, int) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = a; g_xch2[w][l] = b; g_wave[w].wait();
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * (l >> 4) + r, j = l & 15;
        for (int k = 0; k < 4; ++k) c[r] = fmaf(g_xch[w][i + 16 * k], g_xch2[w][j + 16 * k], c[r]);
    }
    g_wave[w].wait(); return c;
}
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a) {
    for (unsigned bz = 0; bz < grid.z; ++bz) for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
        g_block.live = block.x; g_block.waiting = 0;
        for (int w = 0; w < 16; ++w) { g_wave[w].live = 64; g_wave[w].waiting = 0; }
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t) ts.emplace_back([=] {
            threadIdx = dim3(t); blockIdx = dim3(bx, by, bz);
            k(a...);
            g_block.drop(); g_wave[t >> 6].drop();
        });
        for (auto& t : ts) t.join();
    }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, strm, ...) emu_launch(kern, grid, block, __VA_ARGS__)
