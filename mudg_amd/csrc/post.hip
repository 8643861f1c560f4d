// post.hip — per-modality post-processing of decoded frames (byte / integer work, HBM-bound):
//   frames_to_u8      clamp, (x + 1) / 2 * 255, truncate, (b c t h w) fp32 -> (b t h w c) uint8   eval_tools.py:22-27
//   depth_from_u8     mean of the three uint8 channels / 255                                      eval_tools.py:71
//   semantic_nearest  nearest of the 19 palette colours, first minimum wins                       eval_tools.py:309-347
//   log_sheet         the frame sheet of a logged entry: (n c t h w) fp32 -> (t, n h, w, 3) uint8      utils/save_video.py:62-136
// The arithmetic reproduces the reference's fp32 / integer operations one for one: results are bit-equal.
#include "common.h"

namespace {

__constant__ int PAL[19][3] = {{255, 120, 50}, {255, 192, 203}, {255, 255, 0}, {0, 150, 245}, {0, 255, 255}, {255, 127, 0},
                               {255, 0, 0}, {255, 240, 150}, {135, 60, 0}, {160, 32, 240}, {255, 0, 255}, {139, 137, 137},
                               {75, 0, 75}, {150, 240, 80}, {230, 230, 250}, {0, 175, 0}, {0, 255, 127}, {222, 155, 161},
                               {140, 62, 69}};

__global__ __launch_bounds__(256) void frames_to_u8_kernel(const float* __restrict__ V, uint8_t* __restrict__ O, int C, int T,
                                                            int64_t HW, int64_t total) {
    // one thread per output pixel (b, t, p): reads C planes HW*T apart, writes C consecutive bytes
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t p = i % HW, bt = i / HW;
    const int t = (int)(bt % T);
    const int64_t b = bt / T;
    for (int c = 0; c < C; ++c) {
        float x = V[((b * C + c) * T + t) * HW + p];
        x = fminf(fmaxf(x, -1.0f), 1.0f);
        const float g = __fmul_rn(__fdiv_rn(__fadd_rn(x, 1.0f), 2.0f), 255.0f);
        O[i * C + c] = (uint8_t)(int)g;                      // truncation toward zero, g in [0, 255]
    }
}

__global__ __launch_bounds__(256) void depth_from_u8_kernel(const uint8_t* __restrict__ F, float* __restrict__ D, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = __fadd_rn(__fadd_rn((float)F[3 * i], (float)F[3 * i + 1]), (float)F[3 * i + 2]);
    D[i] = __fdiv_rn(__fdiv_rn(s, 3.0f), 255.0f);
}

__global__ __launch_bounds__(256) void semantic_kernel(const uint8_t* __restrict__ I, uint8_t* __restrict__ Vis,
                                                        int64_t* __restrict__ L, int64_t hw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const int r = I[i], g = I[hw + i], b = I[2 * hw + i];
    int best = 0, bd = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 19; ++k) {
        const int dr = r - PAL[k][0], dg = g - PAL[k][1], db = b - PAL[k][2];
        const int d = dr * dr + dg * dg + db * db;
        if (d < bd) { bd = d; best = k; }                    // strict: the first minimum wins, like np.argmin
    }
    L[i] = best;
    Vis[i] = (uint8_t)PAL[best][0]; Vis[hw + i] = (uint8_t)PAL[best][1]; Vis[2 * hw + i] = (uint8_t)PAL[best][2];
}

// The sheet log_local makes of a logged video (utils/save_video.py:91-96: per frame make_grid(nrow=1, padding=0) = the samples
// stacked along the height, a one-channel entry repeated to three; prepare_to_log's clamp before it, 120-136), in the reference's
// fp32 order: clamp, (x + 1) / 2, * 255, truncate.  PX = 4: a thread owns four pixels of a row — C 16-byte loads, one 12-byte
// store; PX = 1 (W % 4 != 0 or unaligned bases): one pixel per thread.
struct u32x3 { uint32_t x, y, z; };

__device__ __forceinline__ uint32_t sheet_byte(float x, int clamp, int rescale) {
    if (clamp) x = fminf(fmaxf(x, -1.0f), 1.0f);
    if (rescale) x = __fdiv_rn(__fadd_rn(x, 1.0f), 2.0f);
    return (uint32_t)(uint8_t)(int)__fmul_rn(x, 255.0f);    // truncation toward zero
}

template <int PX>
__global__ __launch_bounds__(256) void log_sheet_kernel(const float* __restrict__ V, uint8_t* __restrict__ O, int N, int C, int T, int H, int W,
                                                         int clamp, int rescale, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int wq = W / PX;
    const int w = (int)(i % wq) * PX;
    int64_t r = i / wq;
    const int h = (int)(r % H); r /= H;
    const int n = (int)(r % N);
    const int64_t t = r / N;
    const int64_t plane = (int64_t)T * H * W;                                    // one channel of one sample
    const float* src = V + ((int64_t)n * C * T + t) * H * W + (int64_t)h * W + w;
    uint8_t* dst = O + (((t * N + n) * H + h) * W + w) * 3;
    if (PX == 4) {
        f32x4 ch[3];
        ch[0] = *reinterpret_cast<const f32x4*>(src);
        if (C == 3) { ch[1] = *reinterpret_cast<const f32x4*>(src + plane); ch[2] = *reinterpret_cast<const f32x4*>(src + 2 * plane); }
        else { ch[1] = ch[0]; ch[2] = ch[0]; }
        uint32_t b[12];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[3 * e + c] = sheet_byte(ch[c][e], clamp, rescale);
        u32x3 o;
        o.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        o.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        o.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        *reinterpret_cast<u32x3*>(dst) = o;
    } else {
        const float r0 = src[0];
        const float g0 = C == 3 ? src[plane] : r0, b0 = C == 3 ? src[2 * plane] : r0;
        dst[0] = (uint8_t)sheet_byte(r0, clamp, rescale);
        dst[1] = (uint8_t)sheet_byte(g0, clamp, rescale);
        dst[2] = (uint8_t)sheet_byte(b0, clamp, rescale);
    }
}

}  // namespace

extern "C" int mudg_frames_to_u8(const float* video, uint8_t* out, int B, int C, int T, int64_t HW, void* stream) {
    MUDG_REQUIRE(video && out && B > 0 && C > 0 && T > 0 && HW > 0, "mudg_frames_to_u8: bad arguments");
    const int64_t total = (int64_t)B * T * HW;
    hipLaunchKernelGGL(frames_to_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       video, out, C, T, HW, total);
    return mudg_check_launch("mudg_frames_to_u8");
}

extern "C" int mudg_depth_from_u8(const uint8_t* frames, float* depth, int64_t pixels, void* stream) {
    MUDG_REQUIRE(frames && depth && pixels > 0, "mudg_depth_from_u8: bad arguments");
    hipLaunchKernelGGL(depth_from_u8_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       frames, depth, pixels);
    return mudg_check_launch("mudg_depth_from_u8");
}

extern "C" int mudg_semantic_nearest(const uint8_t* img, uint8_t* vis, int64_t* labels, int64_t hw, void* stream) {
    MUDG_REQUIRE(img && vis && labels && hw > 0, "mudg_semantic_nearest: bad arguments");
    hipLaunchKernelGGL(semantic_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       img, vis, labels, hw);
    return mudg_check_launch("mudg_semantic_nearest");
}

extern "C" int mudg_log_sheet(const float* video, uint8_t* out, int N, int C, int T, int H, int W, int clamp, int rescale, void* stream) {
    MUDG_REQUIRE(video && out && N > 0 && T > 0 && H > 0 && W > 0, "mudg_log_sheet: bad arguments");
    MUDG_REQUIRE(C == 1 || C == 3, "mudg_log_sheet: %d channels (grayscale or rgb entries only)", C);
    const bool wide = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(video) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    const int64_t total = (int64_t)T * N * H * (wide ? W / 4 : W);
    MUDG_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "mudg_log_sheet: entry too large");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL(log_sheet_kernel<4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, video, out, N, C, T, H, W, clamp, rescale, total);
    else hipLaunchKernelGGL(log_sheet_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, video, out, N, C, T, H, W, clamp, rescale, total);
    return mudg_check_launch("mudg_log_sheet");
}
