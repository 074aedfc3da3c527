// input.hip — the image input stage of the reference's loader (modules/dataset/dataset.py:15-19,115-139): an RGBA
// rendering [B,Hs,Ws,4] uint8 becomes rgb [B,3,H,W], silhouette [B,1,H,W] fp32 through PIL's Resize (BILINEAR on the
// premultiplied image, 22-bit fixed point, 8-bit rounding after each pass), ColorJitter's three ImageEnhance blends in a
// drawn order and rotate(angle, NEAREST) in 16.16 fixed point.  Every pixel operation is integer arithmetic or fp32 with
// each operation rounded by itself, so the outputs equal PIL's bit for bit (tests/input_ref.py).
//
// Three launches.  input_setup_kernel: one thread per image fixes its draws (given, or Philox), its rotation
// coefficients (fp64) and zeroes its L sum.  input_resize_kernel: a workgroup per 32 x 8 output tile filters the source
// rows of its vertical support horizontally into LDS and vertically out of it, stores the 8-bit resized image and adds
// the tile's part of the L sum the contrast blend needs (the mean of the image as it stands when contrast's turn comes;
// what precedes it is per pixel).  input_finish_kernel: one thread per output pixel gathers through the rotation, blends,
// converts and writes the planes.
//
// Built with -ffp-contract=off; the blends also spell their roundings (__fmul_rn / __fadd_rn / __fdiv_rn).
#include "vpn_common.h"

namespace {

#pragma clang fp contract(off)

constexpr int IN_THREADS = 256;
constexpr int IN_TW = 32, IN_TH = VPN_INPUT_TILE_ROWS;      // output tile of the resize: one pixel per thread in the vertical pass
constexpr int IN_BITS = 22;                      // PIL's PRECISION_BITS for 8-bit channels
constexpr uint32_t IN_STREAM = 0x80000001u;      // Philox counter word 1 (augment.hip: 0x80000000; the sampler: < 1024)
constexpr int IN_MAX_SIDE = 8192;                // 16.16 coordinates stay far inside int32
constexpr size_t IN_MAX_LDS = 65536;
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_NONE = 3;      // 2: saturation
enum { F_JITTER = 1, F_ROTATE = 2, F_NORMALIZE = 4 };

struct ImageParams {       // what the setup launch leaves for the other two, one per image (64 bytes)
    float f[3];            // brightness, contrast, saturation
    int32_t op[3];         // the operation of each turn (OP_NONE: no jitter)
    int32_t a[6];          // 16.16 affine of the gather: xin = (a2 + x a0 + y a1) >> 16, yin = (a5 + x a3 + y a4) >> 16
    int32_t gather;        // 0: the image stays where it is
    int32_t pad[3];
};

inline size_t in_ws_bytes(int B) { return (size_t)B * (sizeof(unsigned long long) + sizeof(ImageParams)); }

__device__ inline int in_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) of one channel: fp32 d + f * (v - d), each operation rounded, clipped when f lies
// outside [0, 1], truncated
__device__ inline int in_blend(int d, int v, float f, bool clip) {
    float t = __fadd_rn((float)d, __fmul_rn(f, (float)(v - d)));
    if (clip) t = t <= 0.0f ? 0.0f : (t >= 255.0f ? 255.0f : t);
    return (int)t;
}

// one ImageEnhance step on a packed RGBA pixel (R in the low byte); alpha is kept
__device__ inline uint32_t in_enhance(uint32_t px, int op, float f, int mean) {
    const int r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
    const int d = op == OP_BRIGHTNESS ? 0 : (op == OP_CONTRAST ? mean : in_luma(r, g, b));
    const bool clip = !(f >= 0.0f && f <= 1.0f);
    return (px & 0xff000000u) | (uint32_t)in_blend(d, r, f, clip) | ((uint32_t)in_blend(d, g, f, clip) << 8) |
           ((uint32_t)in_blend(d, b, f, clip) << 16);
}

__device__ inline float in_factor(const ImageParams& P, int op) {
    return op == OP_BRIGHTNESS ? P.f[0] : (op == OP_CONTRAST ? P.f[1] : P.f[2]);
}

__device__ inline int in_fix(double v) { return (int)floor(v * 65536.0 + 0.5); }

__global__ __launch_bounds__(64) void input_setup_kernel(
    const float* __restrict__ factors, const int32_t* __restrict__ order, const float* __restrict__ angles, uint64_t seed,
    const uint64_t* __restrict__ seed_dev, uint64_t sample_base, int B, int H, int W, int flags,
    unsigned long long* __restrict__ sums, ImageParams* __restrict__ params, float* __restrict__ angles_out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (seed_dev) seed += *seed_dev;
    const uint64_t gb = sample_base + (uint64_t)b;
    ImageParams P;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    const bool drawn = ((flags & F_JITTER) && !factors) || ((flags & F_ROTATE) && !angles);
    if (drawn) vpn::philox4x32_10(0u, IN_STREAM, (uint32_t)gb, (uint32_t)(gb >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const float u0 = (float)(o[0] >> 8) * 5.9604644775390625e-08f, u1 = (float)(o[1] >> 8) * 5.9604644775390625e-08f,
                u2 = (float)(o[2] >> 8) * 5.9604644775390625e-08f, u3 = (float)(o[3] >> 8) * 5.9604644775390625e-08f;
    P.f[0] = P.f[1] = P.f[2] = 1.0f;
    P.op[0] = P.op[1] = P.op[2] = OP_NONE;
    if (flags & F_JITTER) {
        if (factors) {
            P.f[0] = factors[b * 3]; P.f[1] = factors[b * 3 + 1]; P.f[2] = factors[b * 3 + 2];
        } else {
            P.f[0] = fminf(__fadd_rn(0.6f, __fmul_rn(u0, 0.8f)), 1.4f);
            P.f[1] = fminf(__fadd_rn(0.6f, __fmul_rn(u1, 0.8f)), 1.4f);
            P.f[2] = fminf(__fadd_rn(0.6f, __fmul_rn(u2, 0.8f)), 1.4f);
        }
        if (order) {
            const int o0 = order[b * 3], o1 = order[b * 3 + 1], o2 = order[b * 3 + 2];
            P.op[0] = (unsigned)o0 < 3u ? o0 : OP_NONE;       // a value outside 0..2 is a turn without an operation
            P.op[1] = (unsigned)o1 < 3u ? o1 : OP_NONE;
            P.op[2] = (unsigned)o2 < 3u ? o2 : OP_NONE;
        } else {
            // one of the 6 orders, lexicographic: multiply-shift with rejection (Lemire 2019) over the words of slot 1
            uint32_t q[4];
            vpn::philox4x32_10(1u, IN_STREAM, (uint32_t)gb, (uint32_t)(gb >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), q);
            const uint32_t reject = (0u - 6u) % 6u;
            uint32_t idx = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint64_t m = (uint64_t)q[w] * 6u;
                idx = (uint32_t)(m >> 32);
                if ((uint32_t)m >= reject) break;
            }
            const int first = (int)(idx >> 1), lo = first == 0 ? 1 : 0, hi = first == 2 ? 1 : 2;
            P.op[0] = first;
            P.op[1] = (idx & 1u) ? hi : lo;
            P.op[2] = (idx & 1u) ? lo : hi;
        }
    }
    float angle = 0.0f;
    if (flags & F_ROTATE) {
        if (angles) angle = angles[b];
        else {
            angle = __fmul_rn(u3, 360.0f);
            if (!(angle < 360.0f)) angle = 0.0f;
        }
    }
    angles_out[b] = angle;
    // Image.rotate: angle % 360 (the sign of the divisor); 0, 180 and -- on a square image -- 90 and 270 are transposes
    double a = fmod((double)angle, 360.0);
    if (a < 0.0) a += 360.0;
    const int one = 65536, half = 32768;
    P.gather = 1;
    if (!(flags & F_ROTATE) || a == 0.0) {
        P.gather = 0;
        P.a[0] = one; P.a[1] = 0; P.a[2] = half; P.a[3] = 0; P.a[4] = one; P.a[5] = half;
    } else if (a == 180.0) {
        P.a[0] = -one; P.a[1] = 0; P.a[2] = (W - 1) * one + half; P.a[3] = 0; P.a[4] = -one; P.a[5] = (H - 1) * one + half;
    } else if (a == 90.0 && H == W) {
        P.a[0] = 0; P.a[1] = -one; P.a[2] = (W - 1) * one + half; P.a[3] = one; P.a[4] = 0; P.a[5] = half;
    } else if (a == 270.0 && H == W) {
        P.a[0] = 0; P.a[1] = one; P.a[2] = half; P.a[3] = -one; P.a[4] = 0; P.a[5] = (H - 1) * one + half;
    } else {
        // the matrix about (W/2, H/2) in fp64, then PIL's affine_fixed: the pixel centre folded into the offsets, all six
        // rounded to 16.16.  (PIL also rounds sin / cos to 15 decimals first: 5e-16, far below the 16.16 step.)
        const double r = -(a * (3.14159265358979323846 / 180.0));
        const double c = cos(r), s = sin(r), cx = W / 2.0, cy = H / 2.0;
        double m2 = c * -cx + s * -cy + 0.0, m5 = -s * -cx + c * -cy + 0.0;
        m2 += cx; m5 += cy;
        m2 += c * 0.5 + s * 0.5;
        m5 += -s * 0.5 + c * 0.5;
        P.a[0] = in_fix(c); P.a[1] = in_fix(s); P.a[2] = in_fix(m2);
        P.a[3] = in_fix(-s); P.a[4] = in_fix(c); P.a[5] = in_fix(m5);
    }
    P.pad[0] = P.pad[1] = P.pad[2] = 0;
    params[b] = P;
    sums[b] = 0ull;
}

__device__ inline uint32_t in_premultiply(uint32_t px) {
    const uint32_t al = px >> 24;
    uint32_t t = (px & 255u) * al + 128u;
    const uint32_t r = ((t >> 8) + t) >> 8;
    t = ((px >> 8) & 255u) * al + 128u;
    const uint32_t g = ((t >> 8) + t) >> 8;
    t = ((px >> 16) & 255u) * al + 128u;
    const uint32_t b = ((t >> 8) + t) >> 8;
    return (px & 0xff000000u) | r | (g << 8) | (b << 16);
}

__device__ inline uint32_t in_unpremultiply(uint32_t px) {
    const uint32_t al = px >> 24;
    if (al == 0u || al == 255u) return px;
    const uint32_t r = min(255u * (px & 255u) / al, 255u), g = min(255u * ((px >> 8) & 255u) / al, 255u),
                   b = min(255u * ((px >> 16) & 255u) / al, 255u);
    return (px & 0xff000000u) | r | (g << 8) | (b << 16);
}

// PIL's clip8 of a 22-bit fixed-point sum.  Written as an unsigned shift and minimum on purpose: the signed form
// clamp(acc >> 22, 0, 255) of two channels is fused by hipcc into v_ashr_pk_u8_i32, which on gfx950 leaves the upper half
// of its destination register as it was, while the code around it takes that half to be zero (the packed pixel then
// carried bit 21 of an accumulator in its blue channel).  tests/test_input_cpu.py holds the build to this.
__device__ inline uint32_t in_clip8(int acc) {
    return min((uint32_t)max(acc, 0) >> IN_BITS, 255u);
}

// tab: hb [W,2], hk [W,ksh], vb [H,2], vk [H,ksv] int32 (first tap, tap count; round(k 2^22)).  A table entry that
// points outside the source or outside the staged rows is clamped or skipped: the tables are device data.
__global__ __launch_bounds__(IN_THREADS) void input_resize_kernel(
    const uint32_t* __restrict__ src, const int32_t* __restrict__ tab, int ksh, int ksv, int max_rows, int Hs, int Ws,
    int H, int W, int identity, const ImageParams* __restrict__ params, unsigned long long* __restrict__ sums,
    uint32_t* __restrict__ inter) {
    extern __shared__ uint32_t in_rows[];            // [max_rows][IN_TW] horizontally filtered, premultiplied pixels
    const int32_t* hb = tab;
    const int32_t* hk = hb + (size_t)W * 2;
    const int32_t* vb = hk + (size_t)W * ksh;
    const int32_t* vk = vb + (size_t)H * 2;
    const int b = blockIdx.z, tid = threadIdx.x;
    const int tx0 = blockIdx.x * IN_TW, ty0 = blockIdx.y * IN_TH;
    const int ty1 = min(ty0 + IN_TH, H) - 1;
    const int y0 = min(max(vb[ty0 * 2], 0), Hs);
    const int nrows = min(min(max(vb[ty1 * 2] + vb[ty1 * 2 + 1], y0), Hs) - y0, max_rows);
    const uint32_t* img = src + (size_t)b * Hs * Ws;

    for (int i = tid; i < nrows * IN_TW; i += IN_THREADS) {
        const int r = i / IN_TW, c = i - r * IN_TW, x = tx0 + c;
        if (x >= W) continue;
        const int xmin = min(max(hb[x * 2], 0), Ws), n = min(min(hb[x * 2 + 1], ksh), Ws - xmin);
        const uint32_t* row = img + (size_t)(y0 + r) * Ws + xmin;
        const int32_t* k = hk + (size_t)x * ksh;
        int s0 = 1 << (IN_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
        for (int t = 0; t < n; ++t) {
            uint32_t px = row[t];
            if (!identity) px = in_premultiply(px);
            const int w = k[t];
            s0 += (int)(px & 255u) * w; s1 += (int)((px >> 8) & 255u) * w;
            s2 += (int)((px >> 16) & 255u) * w; s3 += (int)(px >> 24) * w;
        }
        in_rows[i] = in_clip8(s0) | (in_clip8(s1) << 8) | (in_clip8(s2) << 16) | (in_clip8(s3) << 24);
    }
    __syncthreads();

    const int c = tid % IN_TW, x = tx0 + c, y = ty0 + tid / IN_TW;
    const ImageParams& P = params[b];
    unsigned lum = 0;
    bool contrast = false;
    if (x < W && y < H) {
        const int ymin = vb[y * 2], n = min(vb[y * 2 + 1], ksv);
        const int32_t* k = vk + (size_t)y * ksv;
        int s0 = 1 << (IN_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
        for (int t = 0; t < n; ++t) {
            const int r = ymin + t - y0;
            if ((unsigned)r >= (unsigned)nrows) continue;
            const uint32_t px = in_rows[r * IN_TW + c];
            const int w = k[t];
            s0 += (int)(px & 255u) * w; s1 += (int)((px >> 8) & 255u) * w;
            s2 += (int)((px >> 16) & 255u) * w; s3 += (int)(px >> 24) * w;
        }
        uint32_t px = in_clip8(s0) | (in_clip8(s1) << 8) | (in_clip8(s2) << 16) | (in_clip8(s3) << 24);
        if (!identity) px = in_unpremultiply(px);
        inter[((size_t)b * H + y) * W + x] = px;
        // what precedes contrast in this image's order is per pixel: apply it, and L of the result goes into the mean
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int op = P.op[i];
            if (op == OP_CONTRAST) contrast = true;
            if (!contrast && op != OP_NONE) px = in_enhance(px, op, in_factor(P, op), 0);
        }
        lum = (unsigned)in_luma(px & 255, (px >> 8) & 255, (px >> 16) & 255);
    }
    if (P.op[0] == OP_CONTRAST || P.op[1] == OP_CONTRAST || P.op[2] == OP_CONTRAST) {      // uniform over the workgroup
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lum += __shfl_xor(lum, o, 64);
        if ((tid & 63) == 0 && lum) atomicAdd(sums + b, (unsigned long long)lum);           // integer: any order, one sum
    }
}

__global__ __launch_bounds__(IN_THREADS) void input_finish_kernel(
    const uint32_t* __restrict__ inter, const ImageParams* __restrict__ params, const unsigned long long* __restrict__ sums,
    int H, int W, int flags, float* __restrict__ rgb, float* __restrict__ sil) {
    const int b = blockIdx.y;
    const unsigned n = (unsigned)H * W, i = blockIdx.x * IN_THREADS + threadIdx.x;
    if (i >= n) return;
    const ImageParams& P = params[b];
    const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * W);
    uint32_t px = 0u;
    bool inside = true;
    int xin = x, yin = y;
    if (P.gather) {
        // PIL walks xx += a0 along a row and a2 += a1 down the rows in int32: the same sums, taken at once
        xin = (int)((uint32_t)P.a[2] + (uint32_t)x * (uint32_t)P.a[0] + (uint32_t)y * (uint32_t)P.a[1]) >> 16;
        yin = (int)((uint32_t)P.a[5] + (uint32_t)x * (uint32_t)P.a[3] + (uint32_t)y * (uint32_t)P.a[4]) >> 16;
        inside = (unsigned)xin < (unsigned)W && (unsigned)yin < (unsigned)H;
    }
    if (inside) {
        px = inter[((size_t)b * H + yin) * W + xin];
        if (P.op[0] != OP_NONE || P.op[1] != OP_NONE || P.op[2] != OP_NONE) {
            // int(mean(L) + 0.5) = (2 sum + n) / (2 n): a float estimate put right in integers (the quotient is <= 255)
            const unsigned long long num = 2ull * sums[b] + n, den = 2ull * n;
            unsigned mean = (unsigned)__fdiv_rn((float)num, (float)den);
            if ((unsigned long long)mean * den > num) --mean;
            if ((unsigned long long)(mean + 1) * den <= num) ++mean;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int op = P.op[t];
                if (op != OP_NONE) px = in_enhance(px, op, in_factor(P, op), (int)mean);
            }
        }
    }
    float r = __fdiv_rn((float)(px & 255u), 255.0f), g = __fdiv_rn((float)((px >> 8) & 255u), 255.0f),
          bl = __fdiv_rn((float)((px >> 16) & 255u), 255.0f);
    if (flags & F_NORMALIZE) {            // also the zero fill of the rotation: Normalize runs on the rotated tensor
        r = __fdiv_rn(__fsub_rn(r, 0.485f), 0.229f);
        g = __fdiv_rn(__fsub_rn(g, 0.456f), 0.224f);
        bl = __fdiv_rn(__fsub_rn(bl, 0.406f), 0.225f);
    }
    float* o = rgb + (size_t)b * 3 * n + i;
    o[0] = r; o[n] = g; o[2 * (size_t)n] = bl;
    sil[(size_t)b * n + i] = __fdiv_rn((float)(px >> 24), 255.0f);
}

}  // namespace

extern "C" size_t vpn_input_ws(int B) { return B > 0 ? in_ws_bytes(B) : 0; }

extern "C" int vpn_prepare_images(const uint8_t* rgba, const int32_t* tables, int ksh, int ksv, int max_rows,
                                  const float* factors, const int32_t* order, const float* angles, uint64_t seed,
                                  const uint64_t* seed_dev, uint64_t sample_base, int B, int Hs, int Ws, int H, int W,
                                  int flags, void* workspace, size_t workspace_bytes, uint8_t* inter, float* rgb,
                                  float* silhouette, float* angles_out, void* stream) {
    if (!rgba || !tables || !workspace || !inter || !rgb || !silhouette || !angles_out) return VPN_E_BADARG;
    if (B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || ksh <= 0 || ksv <= 0 || max_rows <= 0) return VPN_E_BADARG;
    if (flags & ~(F_JITTER | F_ROTATE | F_NORMALIZE)) return VPN_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(rgba) | reinterpret_cast<uintptr_t>(inter)) & 3) return VPN_E_BADARG;      // 4-byte pixels
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return VPN_E_BADARG;
    if (B > 65535 || Hs > IN_MAX_SIDE || Ws > IN_MAX_SIDE || H > IN_MAX_SIDE || W > IN_MAX_SIDE) return VPN_E_TOOBIG;
    if (ksh > 2 * IN_MAX_SIDE + 1 || ksv > 2 * IN_MAX_SIDE + 1) return VPN_E_TOOBIG;
    if ((uint64_t)B * H * W > 0x1fffffffull || (uint64_t)B * Hs * Ws > 0x1fffffffull) return VPN_E_TOOBIG;
    const size_t lds = (size_t)max_rows * IN_TW * sizeof(uint32_t);
    if (lds > IN_MAX_LDS) return VPN_E_TOOBIG;                  // the rows one tile's vertical support spans (a steep reduction)
    if ((H + IN_TH - 1) / IN_TH > 65535) return VPN_E_TOOBIG;
    if (workspace_bytes < in_ws_bytes(B)) return VPN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* sums = static_cast<unsigned long long*>(workspace);
    ImageParams* params = reinterpret_cast<ImageParams*>(sums + B);
    VPN_LAUNCH(input_setup_kernel, dim3((B + 63) / 64), dim3(64), 0, s, factors, order, angles, seed, seed_dev, sample_base, B,
               H, W, flags, sums, params, angles_out);
    VPN_LAUNCH_CHECK();
    VPN_LAUNCH(input_resize_kernel, dim3((W + IN_TW - 1) / IN_TW, (H + IN_TH - 1) / IN_TH, B), dim3(IN_THREADS), lds, s,
               reinterpret_cast<const uint32_t*>(rgba), tables, ksh, ksv, max_rows, Hs, Ws, H, W,
               (Hs == H && Ws == W) ? 1 : 0, params, sums, reinterpret_cast<uint32_t*>(inter));
    VPN_LAUNCH_CHECK();
    const unsigned n = (unsigned)H * W;
    VPN_LAUNCH(input_finish_kernel, dim3((n + IN_THREADS - 1) / IN_THREADS, B), dim3(IN_THREADS), 0, s,
               reinterpret_cast<const uint32_t*>(inter), params, sums, H, W, flags, rgb, silhouette);
    VPN_LAUNCH_CHECK();
    return 0;
}
