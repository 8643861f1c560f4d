// metrics.hip — scores of generated views against the truths that are already on the device.
//   metric_sse        a lane owns four pixels of a frame (blockIdx.y): the integer sum of (a - b)^2 over pixels and channels
//   metric_ssim       a workgroup owns a 32 x 32 output tile of one channel: Wang et al. 2004 with an integer window; the five moments
//                     are exact integers, the formula is fp64 in a stated order, the per-pixel value goes to a 2^-32 grid
//   metric_depth      a lane owns four pixels: n, the sums of |z - y|, (z - y)^2 and |z - y| / y on a 2^-20 grid, the three delta counts
//   metric_confusion  a workgroup owns 4096 pixels: a C x C histogram in LDS, then one global atomic per cell that is not zero
// Every sum is an integer (wave shuffles, LDS across the waves, 64-bit integer atomics per workgroup) and every floating-point operation
// is a single correctly rounded one in a fixed order (no contraction): no output depends on the order of execution, and all of them are
// bit-equal to the numpy definition in tests/metrics_reference.py.  No MFMA operand is touched: the same code in every library build.
#include "common.h"

namespace {

constexpr int MAX_PIXELS = 1 << 24;            // per frame
constexpr double TWO32 = 4294967296.0, INV_TWO32 = 1.0 / 4294967296.0;
constexpr double E_SCALE = 1048576.0;          // depth errors are summed on a 2^-20 grid
constexpr double Z_TOP = 256.0;                // a depth is taken into [0, 256] before it is compared
constexpr double SSIM_C1 = 6.5025, SSIM_C2 = 58.5225;                      // (0.01 * 255)^2, (0.03 * 255)^2

// rint(65536 g_i / sum g), g_i = exp(-(i - 5)^2 / 4.5), the centre tap corrected so that the taps sum to 2^16
#define SSIM_TAPS {67u, 498u, 2359u, 7167u, 13960u, 17434u, 13960u, 7167u, 2359u, 498u, 67u}
constexpr int TAPS = 11, APRON = TAPS - 1;
constexpr int TILE = 32;                       // outputs per side of a workgroup's tile
constexpr int IN = TILE + APRON;               // 42 input rows and columns
constexpr int ROW_WORDS = 12;                  // a staged row of bytes: 48 >= 42, in 32-bit words
constexpr int MOMENTS = 5;                     // Sx, Sy, Sxx, Syy, Sxy
constexpr int OUT_PER_LANE = 4;                // vertical pass: a lane owns four outputs of a column
constexpr int CONF_MAX_CLASSES = 32;
constexpr int CONF_PIXELS = 4096;              // per workgroup
constexpr int DEPTH_SUMS = 8;                  // n, sum e, sum e^2, sum r, three delta counts, one spare

struct u32x3 { uint32_t x, y, z; };

template <typename T>
__device__ __forceinline__ T wave_add(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// PX pixels' twelve or three bytes
template <int PX>
__device__ __forceinline__ void load_bytes(const uint8_t* __restrict__ src, uint32_t (&b)[3 * PX]) {
    if (PX == 4) {
        const u32x3 w = *reinterpret_cast<const u32x3*>(src);
        const uint32_t t[12] = {w.x & 255u, (w.x >> 8) & 255u, (w.x >> 16) & 255u, w.x >> 24, w.y & 255u, (w.y >> 8) & 255u,
                                (w.y >> 16) & 255u, w.y >> 24, w.z & 255u, (w.z >> 8) & 255u, (w.z >> 16) & 255u, w.z >> 24};
#pragma unroll
        for (int e = 0; e < 12; ++e) b[e] = t[e];
    } else {
        b[0] = src[0]; b[1] = src[1]; b[2] = src[2];
    }
}

template <int PX>
__device__ __forceinline__ void load_f32(const float* __restrict__ src, float (&v)[PX]) {
    if (PX == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int e = 0; e < PX; ++e) v[e] = t[e];
    } else {
        v[0] = src[0];
    }
}

// A workgroup covers 256 * PX pixels: its sum is at most 1024 * 3 * 255^2 < 2^28
template <int PX>
__global__ __launch_bounds__(256) void metric_sse_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int hw,
                                                          unsigned long long* __restrict__ sse) {
    __shared__ unsigned part[4];
    const int f = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    unsigned s = 0;
    if (p < hw) {
        const int64_t at = ((int64_t)f * hw + p) * 3;
        uint32_t x[3 * PX], y[3 * PX];
        load_bytes<PX>(a + at, x);
        load_bytes<PX>(b + at, y);
#pragma unroll
        for (int e = 0; e < 3 * PX; ++e) { const int d = (int)x[e] - (int)y[e]; s += (unsigned)(d * d); }
    }
    s = wave_add(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(sse + f, (unsigned long long)s);                    // a workgroup with nothing to add issues no atomic
    }
}

// The rule's formula: every product, sum and quotient a separate correctly rounded operation.  Returns rint(s 2^32), half to even.
__device__ __forceinline__ long long ssim_q(unsigned long long Sx, unsigned long long Sy, unsigned long long Sxx, unsigned long long Syy,
                                            unsigned long long Sxy) {
    const double mx = __dmul_rn(__ull2double_rn(Sx), INV_TWO32), my = __dmul_rn(__ull2double_rn(Sy), INV_TWO32);   // sums below 2^48: exact
    const double mxx = __dmul_rn(mx, mx), myy = __dmul_rn(my, my), mxy = __dmul_rn(mx, my);
    const double vx = __dsub_rn(__dmul_rn(__ull2double_rn(Sxx), INV_TWO32), mxx);
    const double vy = __dsub_rn(__dmul_rn(__ull2double_rn(Syy), INV_TWO32), myy);
    const double cxy = __dsub_rn(__dmul_rn(__ull2double_rn(Sxy), INV_TWO32), mxy);
    const double num = __dmul_rn(__dadd_rn(__dmul_rn(2.0, mxy), SSIM_C1), __dadd_rn(__dmul_rn(2.0, cxy), SSIM_C2));
    const double den = __dmul_rn(__dadd_rn(__dadd_rn(mxx, myy), SSIM_C1), __dadd_rn(__dadd_rn(vx, vy), SSIM_C2));
    return (long long)rint(__dmul_rn(__ddiv_rn(num, den), TWO32));           // |s| <= 1: the product is exact and below 2^33
}

// blockIdx.x = (channel, tile row, tile column), blockIdx.y = frame.  Stage the tile and its 10-pixel apron of both images as bytes;
// horizontal pass: a lane owns four outputs of a row, five uint32 planes (each below 2^32: 255^2 2^16 < 2^32); vertical pass: a lane owns
// four outputs of a column, fourteen rows of each plane, 64-bit sums (below 2^48); the formula; the workgroup's sum of q; one atomic.
// LDS: 2 * 42 * 48 + 5 * 42 * 32 * 4 = 30912 bytes, five workgroups per CU.
__global__ __launch_bounds__(256) void metric_ssim_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W,
                                                           int tiles_x, int tiles_y, unsigned long long* __restrict__ sums) {
    constexpr uint32_t w[TAPS] = SSIM_TAPS;
    __shared__ uint32_t bytes[2][IN * ROW_WORDS];
    __shared__ uint32_t plane[MOMENTS][IN * TILE];
    __shared__ unsigned long long part[4];
    const int f = blockIdx.y;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, ch = blockIdx.x / (tiles_x * tiles_y);
    const int ox = tx * TILE, oy = ty * TILE;                                // the tile's first output = its first input
    const int tid = threadIdx.x;

    uint8_t* stage_a = reinterpret_cast<uint8_t*>(bytes[0]);
    uint8_t* stage_b = reinterpret_cast<uint8_t*>(bytes[1]);
    for (int i = tid; i < IN * IN; i += 256) {
        const int r = i / IN, c = i - r * IN;
        const int gy = oy + r, gx = ox + c;
        uint8_t va = 0, vb = 0;                                              // beyond the frame: zeros, used by no valid output
        if (gy < H && gx < W) {
            const int64_t at = (((int64_t)f * H + gy) * W + gx) * 3 + ch;
            va = a[at];
            vb = b[at];
        }
        stage_a[r * (ROW_WORDS * 4) + c] = va;
        stage_b[r * (ROW_WORDS * 4) + c] = vb;
    }
    __syncthreads();

    for (int i = tid; i < IN * (TILE / 4); i += 256) {
        const int r = i / (TILE / 4), g = i - r * (TILE / 4);               // outputs 4 g .. 4 g + 3 of row r read bytes 4 g .. 4 g + 13
        uint32_t x[16], y[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t wa = bytes[0][r * ROW_WORDS + g + k], wb = bytes[1][r * ROW_WORDS + g + k];
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[4 * k + e] = (wa >> (8 * e)) & 255u; y[4 * k + e] = (wb >> (8 * e)) & 255u; }
        }
        uint32_t xx[14], yy[14], xy[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) { xx[k] = x[k] * x[k]; yy[k] = y[k] * y[k]; xy[k] = x[k] * y[k]; }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            uint32_t s[MOMENTS] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                s[0] += w[k] * x[o + k]; s[1] += w[k] * y[o + k]; s[2] += w[k] * xx[o + k]; s[3] += w[k] * yy[o + k]; s[4] += w[k] * xy[o + k];
            }
#pragma unroll
            for (int m = 0; m < MOMENTS; ++m) plane[m][r * TILE + 4 * g + o] = s[m];
        }
    }
    __syncthreads();

    const int col = tid & (TILE - 1), r0 = (tid >> 5) * OUT_PER_LANE;       // outputs (r0 .. r0 + 3, col) read rows r0 .. r0 + 13
    unsigned long long acc[MOMENTS][OUT_PER_LANE] = {};
#pragma unroll
    for (int r = 0; r < OUT_PER_LANE + APRON; ++r) {
        uint32_t v[MOMENTS];
#pragma unroll
        for (int m = 0; m < MOMENTS; ++m) v[m] = plane[m][(r0 + r) * TILE + col];
#pragma unroll
        for (int o = 0; o < OUT_PER_LANE; ++o) {
            if (r - o >= 0 && r - o < TAPS) {
#pragma unroll
                for (int m = 0; m < MOMENTS; ++m) acc[m][o] += (unsigned long long)w[r - o] * v[m];
            }
        }
    }
    long long q = 0;
#pragma unroll
    for (int o = 0; o < OUT_PER_LANE; ++o) {
        if (oy + r0 + o < H - APRON && ox + col < W - APRON) q += ssim_q(acc[0][o], acc[1][o], acc[2][o], acc[3][o], acc[4][o]);
    }
    unsigned long long u = wave_add((unsigned long long)q);                  // two's complement: the wrapped sum is the signed sum
    if ((tid & 63) == 0) part[tid >> 6] = u;
    __syncthreads();
    if (tid == 0) {
        u = part[0] + part[1] + part[2] + part[3];
        if (u) atomicAdd(sums + f, u);
    }
}

// A workgroup covers 256 * PX pixels: the four counts fit 32 bits; sum e 2^20 <= 2^10 2^28, sum e^2 2^20 <= 2^10 2^36 and
// sum r 2^20 <= 2^10 2^34 do not.
template <int PX>
__global__ __launch_bounds__(256) void metric_depth_kernel(const float* __restrict__ depth, const float* __restrict__ lidar, int hw,
                                                            double min_depth, double max_depth, unsigned long long* __restrict__ sums) {
    __shared__ unsigned s32[4][4];
    __shared__ unsigned long long s64[4][3];
    const int f = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    unsigned n = 0, d1 = 0, d2 = 0, d3 = 0;
    unsigned long long se = 0, see = 0, sr = 0;
    if (p < hw) {
        const int64_t at = (int64_t)f * hw + p;
        float z32[PX], y32[PX];
        load_f32<PX>(depth + at, z32);
        load_f32<PX>(lidar + at, y32);
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const double y = (double)y32[k];
            if (y > min_depth && y < max_depth && z32[k] == z32[k]) {        // not a number: not counted
                const double z = fmin(fmax((double)z32[k], 0.0), Z_TOP);
                const double e = fabs(__dsub_rn(z, y));
                const double r = __ddiv_rn(e, y);
                const double t = fmax(__ddiv_rn(z, y), __ddiv_rn(y, z));     // z = 0: infinity, inside no threshold
                n += 1u;
                se += (unsigned long long)rint(__dmul_rn(e, E_SCALE));
                see += (unsigned long long)rint(__dmul_rn(__dmul_rn(e, e), E_SCALE));
                sr += (unsigned long long)rint(__dmul_rn(r, E_SCALE));
                d1 += t < 1.25 ? 1u : 0u; d2 += t < 1.5625 ? 1u : 0u; d3 += t < 1.953125 ? 1u : 0u;
            }
        }
    }
    n = wave_add(n); d1 = wave_add(d1); d2 = wave_add(d2); d3 = wave_add(d3);
    se = wave_add(se); see = wave_add(see); sr = wave_add(sr);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s32[wave][0] = n; s32[wave][1] = d1; s32[wave][2] = d2; s32[wave][3] = d3;
        s64[wave][0] = se; s64[wave][1] = see; s64[wave][2] = sr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        n = s32[0][0] + s32[1][0] + s32[2][0] + s32[3][0];
        if (n) {
            unsigned long long* s = sums + (int64_t)f * DEPTH_SUMS;
            atomicAdd(s + 0, (unsigned long long)n);
            atomicAdd(s + 1, s64[0][0] + s64[1][0] + s64[2][0] + s64[3][0]);
            atomicAdd(s + 2, s64[0][1] + s64[1][1] + s64[2][1] + s64[3][1]);
            atomicAdd(s + 3, s64[0][2] + s64[1][2] + s64[2][2] + s64[3][2]);
            atomicAdd(s + 4, (unsigned long long)(s32[0][1] + s32[1][1] + s32[2][1] + s32[3][1]));
            atomicAdd(s + 5, (unsigned long long)(s32[0][2] + s32[1][2] + s32[2][2] + s32[3][2]));
            atomicAdd(s + 6, (unsigned long long)(s32[0][3] + s32[1][3] + s32[2][3] + s32[3][3]));
        }
    }
}

// cell[gt][pred] counts of up to 4096 pixels in LDS (32-bit integer atomics), cell C * C the predictions outside [0, C)
__global__ __launch_bounds__(256) void metric_confusion_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int hw,
                                                                int classes, unsigned long long* __restrict__ confusion,
                                                                unsigned long long* __restrict__ bad) {
    __shared__ unsigned cell[CONF_MAX_CLASSES * CONF_MAX_CLASSES + 1];
    const int f = blockIdx.y, cells = classes * classes;
    for (int i = threadIdx.x; i <= cells; i += 256) cell[i] = 0u;
    __syncthreads();
    const int first = blockIdx.x * CONF_PIXELS;
    const int end = first + CONF_PIXELS < hw ? first + CONF_PIXELS : hw;
    for (int p = first + threadIdx.x; p < end; p += 256) {
        const int64_t at = (int64_t)f * hw + p;
        const int64_t g = gt[at], q = pred[at];
        if (g >= 0 && g < classes) atomicAdd(&cell[(q >= 0 && q < classes) ? (int)g * classes + (int)q : cells], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= cells; i += 256) {
        const unsigned v = cell[i];
        if (v) atomicAdd(i < cells ? confusion + (int64_t)f * cells + i : bad + f, (unsigned long long)v);
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool shape_ok(int frames, int H, int W) { return frames > 0 && frames <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= MAX_PIXELS; }
inline dim3 frame_grid(int frames, int hw, int px) { return dim3((unsigned)((hw / px + 255) / 256), (unsigned)frames); }

}  // namespace

extern "C" int mudg_metric_sse(const uint8_t* a_u8, const uint8_t* b_u8, int frames, int H, int W, uint64_t* sse, void* stream) {
    MUDG_REQUIRE(a_u8 && b_u8 && sse, "mudg_metric_sse: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_metric_sse: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    const int hw = H * W;
    const bool wide = (W & 3) == 0 && aligned4(a_u8) && aligned4(b_u8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sse);
    if (wide) hipLaunchKernelGGL(metric_sse_kernel<4>, frame_grid(frames, hw, 4), dim3(256), 0, s, a_u8, b_u8, hw, out);
    else hipLaunchKernelGGL(metric_sse_kernel<1>, frame_grid(frames, hw, 1), dim3(256), 0, s, a_u8, b_u8, hw, out);
    return mudg_check_launch("mudg_metric_sse");
}

extern "C" int mudg_metric_ssim(const uint8_t* a_u8, const uint8_t* b_u8, int frames, int H, int W, int64_t* sums, void* stream) {
    MUDG_REQUIRE(a_u8 && b_u8 && sums, "mudg_metric_ssim: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_metric_ssim: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    MUDG_REQUIRE(H >= TAPS && W >= TAPS, "mudg_metric_ssim: %d x %d frames (the 11 x 11 window needs at least 11 x 11)", H, W);
    const int tiles_x = (W - APRON + TILE - 1) / TILE, tiles_y = (H - APRON + TILE - 1) / TILE;
    hipLaunchKernelGGL(metric_ssim_kernel, dim3((unsigned)(3 * tiles_x * tiles_y), (unsigned)frames), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       a_u8, b_u8, H, W, tiles_x, tiles_y, reinterpret_cast<unsigned long long*>(sums));
    return mudg_check_launch("mudg_metric_ssim");
}

extern "C" int mudg_metric_depth(const float* depth, const float* lidar, int frames, int H, int W, double min_depth, double max_depth,
                                 int64_t* sums, void* stream) {
    MUDG_REQUIRE(depth && lidar && sums, "mudg_metric_depth: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_metric_depth: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    MUDG_REQUIRE(min_depth >= 0.015625 && max_depth <= 256.0 && min_depth < max_depth,
                 "mudg_metric_depth: depth range (%g, %g) (2^-6 <= min_depth < max_depth <= 256: the headroom of the sums)", min_depth, max_depth);
    const int hw = H * W;
    const bool wide = (W & 3) == 0 && aligned16(depth) && aligned16(lidar);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
    if (wide) hipLaunchKernelGGL(metric_depth_kernel<4>, frame_grid(frames, hw, 4), dim3(256), 0, s, depth, lidar, hw, min_depth, max_depth, out);
    else hipLaunchKernelGGL(metric_depth_kernel<1>, frame_grid(frames, hw, 1), dim3(256), 0, s, depth, lidar, hw, min_depth, max_depth, out);
    return mudg_check_launch("mudg_metric_depth");
}

extern "C" int mudg_metric_confusion(const int64_t* pred, const int64_t* gt, int frames, int H, int W, int classes, int64_t* confusion,
                                     int64_t* bad, void* stream) {
    MUDG_REQUIRE(pred && gt && confusion && bad, "mudg_metric_confusion: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_metric_confusion: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    MUDG_REQUIRE(classes > 0 && classes <= CONF_MAX_CLASSES, "mudg_metric_confusion: %d classes (1 .. 32)", classes);
    const int hw = H * W;
    hipLaunchKernelGGL(metric_confusion_kernel, dim3((unsigned)((hw + CONF_PIXELS - 1) / CONF_PIXELS), (unsigned)frames), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), pred, gt, hw, classes, reinterpret_cast<unsigned long long*>(confusion),
                       reinterpret_cast<unsigned long long*>(bad));
    return mudg_check_launch("mudg_metric_confusion");
}
