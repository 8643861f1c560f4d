// depth.hip — metric depth from the generated depth stream, and generated views lifted to points.
//   depth_align_sums   a lane owns four pixels of a row of one frame (blockIdx.y): the five integer sums of the least-squares line
//                      lidar ~ m depth + c over the pixels where both are positive; wave shuffles, LDS across the waves, one set of
//                      64-bit integer atomics per workgroup                                       data_process/depthlab_tools.py:114-136
//   depth_align_solve  a lane owns a frame: the line from the sums, fp64 in a stated order
//   depth_finish       z = m (k / 765) + c, 100 m on sky, clipped to [0, 100]; optionally the Spectral picture of z / 100
//                                                                        depthlab_tools.py:67-87, virtual_render/eval_tools.py:137-306
//   colormap_spectral  the picture rule on its own: eleven table colours and a linear blend, fp32 operation for operation
//   depth_unproject    a pixel of a view with its depth to a packed world-space point (§12's format) and a validity byte
// Every sum is an integer and every floating-point operation is a single correctly rounded one in a fixed order (no contraction): no
// output depends on the order of execution, and all of them are bit-equal to the numpy definition in tests/depth_reference.py.
// PX = 4: a lane owns four consecutive pixels of a row — 12 bytes of uint8 frame, one 16-byte fp32 access; PX = 1 (W % 4 != 0 or
// unaligned bases): one pixel per lane.  Per-frame tables are indexed by blockIdx.y alone: uniform addresses, scalar loads.
#include "depth_shared.h"

namespace {

constexpr double Q_SCALE = 1048576.0;          // LiDAR depths are summed on a 2^-20 m grid
constexpr double K_FULL = 765.0;               // r + g + b of a white pixel: the stream's depth is k / 765
constexpr int SUMS = 5;                        // n, sum k, sum k^2, sum q, sum k q
constexpr int TABLE_DOUBLES = 16;              // c2w[12], fx, fy, cx, cy

// matplotlib's Spectral, eleven triples (eval_tools.py:170-182), rounded to fp32
__constant__ float SPECTRAL[11][3] = {{0.61960784313725492f, 0.003921568627450980f, 0.25882352941176473f},
                                      {0.83529411764705885f, 0.24313725490196078f, 0.30980392156862746f},
                                      {0.95686274509803926f, 0.42745098039215684f, 0.2627450980392157f},
                                      {0.99215686274509807f, 0.68235294117647061f, 0.38039215686274508f},
                                      {0.99607843137254903f, 0.8784313725490196f, 0.54509803921568623f},
                                      {1.0f, 1.0f, 0.74901960784313726f},
                                      {0.90196078431372551f, 0.96078431372549022f, 0.59607843137254901f},
                                      {0.6705882352941176f, 0.8666666666666667f, 0.64313725490196083f},
                                      {0.4f, 0.76078431372549016f, 0.6470588235294118f},
                                      {0.19607843137254902f, 0.53333333333333333f, 0.74117647058823533f},
                                      {0.36862745098039218f, 0.30980392156862746f, 0.63529411764705879f}};

// method_custom (eval_tools.py:230-241) on a value already taken to [0, 1]'s scale: the three blended colours, fp32
__device__ __forceinline__ void spectral(float x, int reversed, float (&out)[3]) {
    const float pos = __fmul_rn(fminf(fmaxf(x, 0.0f), 1.0f), 10.0f);         // not a number: 0
    const int left = (int)pos;
    const int right = left + 1 < 10 ? left + 1 : 10;
    const float d = __fsub_rn(pos, (float)left);
    const float* L = SPECTRAL[reversed ? 10 - left : left];
    const float* R = SPECTRAL[reversed ? 10 - right : right];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, d), L[c]), __fmul_rn(d, R[c]));
}
__device__ __forceinline__ uint32_t colour_byte(float v) { return (uint32_t)(uint8_t)(int)__fmul_rn(v, 255.0f); }   // truncation, v in [0, 1]

// PX pixels of a frame: k = r + g + b each
template <int PX>
__device__ __forceinline__ void load_k(const uint8_t* __restrict__ src, int (&k)[PX]) {
    if (PX == 4) {
        const u32x3 w = *reinterpret_cast<const u32x3*>(src);
        const uint32_t b[12] = {w.x & 255u, (w.x >> 8) & 255u, (w.x >> 16) & 255u, w.x >> 24, w.y & 255u, (w.y >> 8) & 255u,
                                (w.y >> 16) & 255u, w.y >> 24, w.z & 255u, (w.z >> 8) & 255u, (w.z >> 16) & 255u, w.z >> 24};
#pragma unroll
        for (int e = 0; e < PX; ++e) k[e] = (int)(b[3 * e] + b[3 * e + 1] + b[3 * e + 2]);
    } else {
        k[0] = (int)src[0] + (int)src[1] + (int)src[2];
    }
}

template <typename T>
__device__ __forceinline__ T wave_add(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// A workgroup covers 256 * PX pixels: n <= 2^10, sum k < 2^20 and sum k^2 < 2^30 fit 32 bits; sum q < 2^38 and sum k q < 2^48 do not.
template <int PX>
__global__ __launch_bounds__(256) void depth_align_sums_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ lidar,
                                                                int hw, unsigned long long* __restrict__ sums) {
    __shared__ unsigned s32[4][3];
    __shared__ unsigned long long s64[4][2];
    const int f = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;                     // the lane's first pixel of the frame
    unsigned n = 0, sk = 0, skk = 0;
    unsigned long long sq = 0, skq = 0;
    if (p < hw) {
        const int64_t at = (int64_t)f * hw + p;
        int k[PX];
        float y[PX];
        load_k<PX>(frames + at * 3, k);
        load_f32<PX>(lidar + at, y);
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            if (k[e] > 0 && y[e] > 0.0f && y[e] < 256.0f) {
                const unsigned long long q = (unsigned long long)rint(__dmul_rn((double)y[e], Q_SCALE));   // exact product, half to even
                n += 1u; sk += (unsigned)k[e]; skk += (unsigned)(k[e] * k[e]);
                sq += q; skq += (unsigned long long)k[e] * q;
            }
        }
    }
    n = wave_add(n); sk = wave_add(sk); skk = wave_add(skk); sq = wave_add(sq); skq = wave_add(skq);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s32[wave][0] = n; s32[wave][1] = sk; s32[wave][2] = skk; s64[wave][0] = sq; s64[wave][1] = skq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        n = s32[0][0] + s32[1][0] + s32[2][0] + s32[3][0];
        if (n) {                                                             // a workgroup with nothing to add issues no atomic
            unsigned long long* s = sums + (int64_t)f * SUMS;
            atomicAdd(s + 0, (unsigned long long)n);
            atomicAdd(s + 1, (unsigned long long)(s32[0][1] + s32[1][1] + s32[2][1] + s32[3][1]));
            atomicAdd(s + 2, (unsigned long long)(s32[0][2] + s32[1][2] + s32[2][2] + s32[3][2]));
            atomicAdd(s + 3, s64[0][0] + s64[1][0] + s64[2][0] + s64[3][0]);
            atomicAdd(s + 4, s64[0][1] + s64[1][1] + s64[2][1] + s64[3][1]);
        }
    }
}

__global__ __launch_bounds__(64) void depth_align_solve_kernel(const unsigned long long* __restrict__ sums, int frames,
                                                                double* __restrict__ coef, uint8_t* __restrict__ fitted) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= frames) return;
    const unsigned long long* s = sums + (int64_t)f * SUMS;
    const unsigned long long n = s[0];
    const double N = __ull2double_rn(n), Sk = __ull2double_rn(s[1]), Skk = __ull2double_rn(s[2]), Sq = __ull2double_rn(s[3]), Skq = __ull2double_rn(s[4]);
    const double den = __dsub_rn(__dmul_rn(N, Skk), __dmul_rn(Sk, Sk));
    double m = 100.0, c = 0.0;                                               // not fitted: the stream's own scale (100 m)
    const bool fit = n >= 2 && den > 0.0;
    if (fit) {
        const double m1 = __ddiv_rn(__dsub_rn(__dmul_rn(N, Skq), __dmul_rn(Sk, Sq)), den);
        const double c1 = __ddiv_rn(__dsub_rn(Sq, __dmul_rn(m1, Sk)), N);
        m = __ddiv_rn(__dmul_rn(m1, K_FULL), Q_SCALE);
        c = __ddiv_rn(c1, Q_SCALE);
    }
    coef[2 * f] = m;
    coef[2 * f + 1] = c;
    fitted[f] = fit ? 1 : 0;
}

template <int PX>
__global__ __launch_bounds__(256) void depth_finish_kernel(const uint8_t* __restrict__ frames, const double* __restrict__ coef,
                                                            const int64_t* __restrict__ labels, long long sky_label, int hw,
                                                            float* __restrict__ depth, uint8_t* __restrict__ vis) {
    const int f = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    if (p >= hw) return;
    const double m = coef[2 * f], c = coef[2 * f + 1];
    const int64_t at = (int64_t)f * hw + p;
    int k[PX];
    bool sky[PX];
    load_k<PX>(frames + at * 3, k);
    load_sky<PX>(labels, at, sky_label, sky);
    float z32[PX];
    uint32_t b[3 * PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        double z = __dadd_rn(__dmul_rn(m, __ddiv_rn((double)k[e], K_FULL)), c);
        if (sky[e]) z = 100.0;
        z = fmin(fmax(z, 0.0), 100.0);
        z32[e] = __double2float_rn(z);
        if (vis) {
            float col[3];
            spectral(__fdiv_rn(z32[e], 100.0f), 0, col);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) b[3 * e + ch] = colour_byte(col[ch]);
        }
    }
    if (PX == 4) {
        const f32x4 o = {z32[0], z32[1], z32[2], z32[3]};
        *reinterpret_cast<f32x4*>(depth + at) = o;
        if (vis) {
            u32x3 w;
            w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            *reinterpret_cast<u32x3*>(vis + at * 3) = w;
        }
    } else {
        depth[at] = z32[0];
        if (vis) { vis[at * 3] = (uint8_t)b[0]; vis[at * 3 + 1] = (uint8_t)b[1]; vis[at * 3 + 2] = (uint8_t)b[2]; }
    }
}

// lo = fp32(val_min), den = fp32(val_max - val_min) as visualize_depth forms them (eval_tools.py:297-298); rescale = the range is not (0, 1)
__global__ __launch_bounds__(256) void colormap_spectral_kernel(const float* __restrict__ values, int64_t n, int rescale, float lo, float den,
                                                                 int reversed, uint8_t* __restrict__ bytes, float* __restrict__ colours) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float x = values[i];
    if (rescale) x = __fdiv_rn(__fsub_rn(x, lo), den);
    float col[3];
    spectral(x, reversed, col);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (bytes) bytes[3 * i + ch] = (uint8_t)colour_byte(col[ch]);
        if (colours) colours[3 * i + ch] = col[ch];
    }
}

template <int PX>
__global__ __launch_bounds__(256) void depth_unproject_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                                               const int64_t* __restrict__ labels, long long sky_label,
                                                               const double* __restrict__ table, int hw, int W, double min_depth,
                                                               double max_depth, u32x4* __restrict__ points, uint8_t* __restrict__ valid) {
    const int f = blockIdx.y;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    if (p >= hw) return;
    const double* t = table + (int64_t)f * TABLE_DOUBLES;
    const double fx = t[12], fy = t[13], cx = t[14], cy = t[15];
    const int64_t at = (int64_t)f * hw + p;
    const int j = p / W, i0 = p - j * W;                                     // PX = 4: W % 4 == 0, the four pixels share the row
    float z32[PX];
    bool sky[PX];
    uint32_t colour[PX];
    load_f32<PX>(depth + at, z32);
    load_sky<PX>(labels, at, sky_label, sky);
    if (PX == 4) {
        const u32x3 w = *reinterpret_cast<const u32x3*>(rgb + at * 3);
        colour[0] = w.x & 0xffffffu;
        colour[1] = (w.x >> 24) | ((w.y & 0xffffu) << 8);
        colour[2] = (w.y >> 16) | ((w.z & 0xffu) << 16);
        colour[3] = w.z >> 8;
    } else {
        colour[0] = (uint32_t)rgb[at * 3] | ((uint32_t)rgb[at * 3 + 1] << 8) | ((uint32_t)rgb[at * 3 + 2] << 16);
    }
    const double yn = __ddiv_rn(__dsub_rn(__dadd_rn((double)j, 0.5), cy), fy);
    uint32_t ok[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        const double z = (double)z32[e];
        const double xn = __ddiv_rn(__dsub_rn(__dadd_rn((double)(i0 + e), 0.5), cx), fx);
        const double xc = __dmul_rn(xn, z), yc = __dmul_rn(yn, z);
        ok[e] = (z > min_depth && z < max_depth && !sky[e]) ? 1u : 0u;       // not a number: not valid
        u32x4 q = {0u, 0u, 0u, 0u};                                          // a pixel that is not valid stores zeros
        if (ok[e]) {
            q.x = __float_as_uint(__double2float_rn(row4(t, xc, yc, z)));
            q.y = __float_as_uint(__double2float_rn(row4(t + 4, xc, yc, z)));
            q.z = __float_as_uint(__double2float_rn(row4(t + 8, xc, yc, z)));
            q.w = colour[e];
        }
        points[at + e] = q;
    }
    if (PX == 4) *reinterpret_cast<uint32_t*>(valid + at) = ok[0] | (ok[1] << 8) | (ok[2] << 16) | (ok[3] << 24);
    else valid[at] = (uint8_t)ok[0];
}

}  // namespace

extern "C" int mudg_depth_align_sums(const uint8_t* frames_u8, const float* lidar, int frames, int H, int W, uint64_t* sums, void* stream) {
    MUDG_REQUIRE(frames_u8 && lidar && sums, "mudg_depth_align_sums: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_depth_align_sums: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    const int hw = H * W;
    const bool wide = (W & 3) == 0 && aligned4(frames_u8) && aligned16(lidar);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
    if (wide) hipLaunchKernelGGL(depth_align_sums_kernel<4>, frame_grid(frames, hw, 4), dim3(256), 0, s, frames_u8, lidar, hw, out);
    else hipLaunchKernelGGL(depth_align_sums_kernel<1>, frame_grid(frames, hw, 1), dim3(256), 0, s, frames_u8, lidar, hw, out);
    return mudg_check_launch("mudg_depth_align_sums");
}

extern "C" int mudg_depth_align_solve(const uint64_t* sums, int frames, double* coef, uint8_t* fitted, void* stream) {
    MUDG_REQUIRE(sums && coef && fitted, "mudg_depth_align_solve: null argument");
    MUDG_REQUIRE(frames > 0 && frames <= 65535, "mudg_depth_align_solve: %d frames", frames);
    hipLaunchKernelGGL(depth_align_solve_kernel, dim3((unsigned)((frames + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(sums), frames, coef, fitted);
    return mudg_check_launch("mudg_depth_align_solve");
}

extern "C" int mudg_depth_finish(const uint8_t* frames_u8, const double* coef, const int64_t* labels, int64_t sky_label, int frames, int H,
                                 int W, float* depth, uint8_t* vis, void* stream) {
    MUDG_REQUIRE(frames_u8 && coef && depth, "mudg_depth_finish: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_depth_finish: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    const int hw = H * W;
    const bool wide = (W & 3) == 0 && aligned4(frames_u8) && aligned16(depth) && aligned4(vis) && aligned16(labels);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL(depth_finish_kernel<4>, frame_grid(frames, hw, 4), dim3(256), 0, s, frames_u8, coef, labels, (long long)sky_label, hw, depth, vis);
    else hipLaunchKernelGGL(depth_finish_kernel<1>, frame_grid(frames, hw, 1), dim3(256), 0, s, frames_u8, coef, labels, (long long)sky_label, hw, depth, vis);
    return mudg_check_launch("mudg_depth_finish");
}

extern "C" int mudg_colormap_spectral(const float* values, int64_t n, double val_min, double val_max, int reversed, uint8_t* bytes,
                                      float* colours, void* stream) {
    MUDG_REQUIRE(values && (bytes || colours), "mudg_colormap_spectral: null argument");
    MUDG_REQUIRE(n > 0 && (n + 255) / 256 <= 0x7fffffffLL, "mudg_colormap_spectral: %lld values", (long long)n);
    MUDG_REQUIRE(val_max > val_min, "mudg_colormap_spectral: invalid values range [%g, %g]", val_min, val_max);
    const int rescale = val_min != 0.0 || val_max != 1.0;
    hipLaunchKernelGGL(colormap_spectral_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), values, n,
                       rescale, (float)val_min, (float)(val_max - val_min), reversed ? 1 : 0, bytes, colours);
    return mudg_check_launch("mudg_colormap_spectral");
}

extern "C" int mudg_depth_unproject(const float* depth, const uint8_t* rgb, const int64_t* labels, int64_t sky_label, const double* table,
                                    int frames, int H, int W, double min_depth, double max_depth, void* points, uint8_t* valid, void* stream) {
    MUDG_REQUIRE(depth && rgb && table && points && valid, "mudg_depth_unproject: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_depth_unproject: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    MUDG_REQUIRE(aligned16(points), "mudg_depth_unproject: unaligned points");
    const int hw = H * W;
    const bool wide = (W & 3) == 0 && aligned16(depth) && aligned4(rgb) && aligned16(labels) && aligned4(valid);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    u32x4* out = reinterpret_cast<u32x4*>(points);
    if (wide) hipLaunchKernelGGL(depth_unproject_kernel<4>, frame_grid(frames, hw, 4), dim3(256), 0, s, depth, rgb, labels, (long long)sky_label, table, hw, W, min_depth, max_depth, out, valid);
    else hipLaunchKernelGGL(depth_unproject_kernel<1>, frame_grid(frames, hw, 1), dim3(256), 0, s, depth, rgb, labels, (long long)sky_label, table, hw, W, min_depth, max_depth, out, valid);
    return mudg_check_launch("mudg_depth_unproject");
}
