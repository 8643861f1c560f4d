// frames.hip — camera, depth and label frames resized into the clips the model takes (memory-bound gathers):
//   resize_u8     (T, H0, W0, C) uint8 -> (T, H, W, C): the 8-bit linear rule or nearest; with the label palette, class ids
//                 (T, H0, W0) -> the resized colour-mapped map (T, H, W, 3)          lvdm/data/waymo_data.py:78-93, data_tools.py:7-215
//   resize_f32    (T, H0, W0) fp32 -> (T, H, W): the fp32 linear rule                  waymo_data.py:300-301 (the depth maps)
//   dense_stream  one resize and the loaders' normalisation, written as three fp32 planes per frame at any place of a
//                 (.., 3, T, H, W) tensor: colour, semantic (ids coloured on the taps) or depth   waymo_data.py:95-118, 305-330
// The sample positions and coefficients are tables the host made (ops.py): a kernel computes no coordinate.  blockIdx = (row segment,
// output row, frame); a lane owns four adjacent output pixels, its two source rows serve all three channels.  WIDE: W % 4 == 0 and
// aligned bases, 16-byte stores of the fp32 planes (12 / 4-byte stores of the bytes); otherwise one bounds-checked store per value.
// Every floating-point operation is a single correctly rounded one in a stated order and the 8-bit rule is integer: results are bit-equal
// to tests/frames_reference.py and between runs.  No MFMA operand is touched: the same code in every library build.
#include "frames_shared.h"

namespace {

constexpr int BLOCK = 128;                     // lanes per workgroup: 512 output pixels of one row
constexpr int PX = 4;                          // output pixels per lane
constexpr int PAL_COLOURS = 21;

// data_process/tools/semantic_tools.py:47-69; rows 0 .. 18 are post.hip's PAL (tests/test_frames_gpu.py ties the two), row 21 serves
// every id above 20
__constant__ int PAL21[PAL_COLOURS + 1][3] = {{255, 120, 50}, {255, 192, 203}, {255, 255, 0}, {0, 150, 245}, {0, 255, 255}, {255, 127, 0},
                                              {255, 0, 0}, {255, 240, 150}, {135, 60, 0}, {160, 32, 240}, {255, 0, 255}, {139, 137, 137},
                                              {75, 0, 75}, {150, 240, 80}, {230, 230, 250}, {0, 175, 0}, {0, 255, 127}, {222, 155, 161},
                                              {140, 62, 69}, {227, 164, 30}, {0, 128, 0}, {0, 0, 0}};

enum { OP_U8_LINEAR = 0, OP_U8_NEAREST = 1, OP_F32 = 2, OP_STREAM_U8 = 3, OP_STREAM_DEPTH = 4 };

struct FramesArgs {
    const void* src;           // (T, H0, W0, CS) uint8 or (T, H0, W0) fp32
    const Tap* xt;             // W entries
    const Tap* yt;             // H entries
    const float* norm;         // 256 entries: (v / 255 - 0.5) * 2 as the host computed it (streams of bytes)
    void* dst;                 // bytes (T, H, W, C), fp32 (T, H, W), or the first fp32 plane of a stream
    uint8_t* u8;               // a stream's optional (T, H, W, 3) bytes
    int H0, W0, CS, C, H, W;   // CS: bytes per source pixel; C: values per output pixel
    int palette;               // CS = 1 ids -> three channels on the taps
    int64_t cs, fs;            // a stream's channel and frame strides, in floats
};

struct u32x3 { uint32_t x, y, z; };

// the C values (three with the palette) of source pixel x of a row
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ row, int x, int CS, int palette, int (&p)[3]) {
    if (palette) {
        const int id = min((int)row[x], PAL_COLOURS);
        p[0] = PAL21[id][0]; p[1] = PAL21[id][1]; p[2] = PAL21[id][2];
    } else if (CS == 3) {
        p[0] = row[3 * (int64_t)x]; p[1] = row[3 * (int64_t)x + 1]; p[2] = row[3 * (int64_t)x + 2];
    } else {
        p[0] = p[1] = p[2] = row[x];
    }
}

// The 8-bit linear rule: horizontal pass in int32 with 11-bit coefficients, vertical pass with the intermediate cut to 2^-7 grey levels
__device__ __forceinline__ int linear_u8(int s00, int s01, int s10, int s11, const Tap& tx, const Tap& ty) {
    const int r0 = s00 * tx.c0 + s01 * tx.c1, r1 = s10 * tx.c0 + s11 * tx.c1;
    return (((ty.c0 * (r0 >> 4)) >> 16) + ((ty.c1 * (r1 >> 4)) >> 16) + 2) >> 2;
}

// clamp(0, 100) / 100, - 0.5, * 2 (waymo_data.py:328-329); a NaN stays one, as in torch.clamp
__device__ __forceinline__ float depth_norm(float d) {
    d = d < 0.0f ? 0.0f : (d > 100.0f ? 100.0f : d);
    return __fmul_rn(__fsub_rn(__fdiv_rn(d, 100.0f), 0.5f), 2.0f);
}

template <int OP, bool WIDE>
__global__ __launch_bounds__(BLOCK) void frames_kernel(const FramesArgs a) {
    const int x0 = (blockIdx.x * BLOCK + threadIdx.x) * PX;
    if (x0 >= a.W) return;
    const int y = blockIdx.y;
    const int64_t t = blockIdx.z;
    Tap ty = a.yt[y];
    ty.s0 = inside(ty.s0, a.H0); ty.s1 = inside(ty.s1, a.H0);
    const int n = WIDE ? PX : min(PX, a.W - x0);                              // WIDE: W % 4 == 0, all four exist
    Tap tx[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        tx[e] = a.xt[min(x0 + e, a.W - 1)];
        tx[e].s0 = inside(tx[e].s0, a.W0); tx[e].s1 = inside(tx[e].s1, a.W0);
    }
    const int64_t out_px = (t * a.H + y) * a.W + x0;                          // the lane's first pixel of a (T, H, W) output

    if (OP == OP_F32 || OP == OP_STREAM_DEPTH) {
        const float* src = static_cast<const float*>(a.src) + t * a.H0 * a.W0;
        const float* row0 = src + (int64_t)ty.s0 * a.W0;
        const float* row1 = src + (int64_t)ty.s1 * a.W0;
        float v[PX];
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            v[e] = linear_f32(row0[tx[e].s0], row0[tx[e].s1], row1[tx[e].s0], row1[tx[e].s1], tx[e], ty);
            if (OP == OP_STREAM_DEPTH) v[e] = depth_norm(v[e]);
        }
        float* dst = static_cast<float*>(a.dst) + (OP == OP_F32 ? out_px : t * a.fs + (int64_t)y * a.W + x0);
        const int planes = OP == OP_F32 ? 1 : 3;                              // the same value in all three channels
        for (int c = 0; c < planes; ++c) {
            float* d = dst + c * a.cs;
            if (WIDE) {
                f32x4 o = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(d) = o;
            } else {
#pragma unroll
                for (int e = 0; e < PX; ++e)
                    if (e < n) d[e] = v[e];
            }
        }
        return;
    }

    // bytes in: the four taps of every pixel once, then the channels
    const uint8_t* src = static_cast<const uint8_t*>(a.src) + t * a.H0 * a.W0 * a.CS;
    const uint8_t* row0 = src + (int64_t)ty.s0 * a.W0 * a.CS;
    const uint8_t* row1 = src + (int64_t)ty.s1 * a.W0 * a.CS;
    int v[PX][3];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        int p00[3];
        load_px(row0, tx[e].s0, a.CS, a.palette, p00);
        if (OP == OP_U8_NEAREST) {
            v[e][0] = p00[0]; v[e][1] = p00[1]; v[e][2] = p00[2];
        } else {
            int p01[3], p10[3], p11[3];
            load_px(row0, tx[e].s1, a.CS, a.palette, p01);
            load_px(row1, tx[e].s0, a.CS, a.palette, p10);
            load_px(row1, tx[e].s1, a.CS, a.palette, p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[e][c] = linear_u8(p00[c], p01[c], p10[c], p11[c], tx[e], ty);
        }
    }

    if (OP == OP_STREAM_U8) {
        float* dst = static_cast<float*>(a.dst) + t * a.fs + (int64_t)y * a.W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = dst + c * a.cs;
            if (WIDE) {
                f32x4 o = {a.norm[v[0][c]], a.norm[v[1][c]], a.norm[v[2][c]], a.norm[v[3][c]]};
                *reinterpret_cast<f32x4*>(d) = o;
            } else {
#pragma unroll
                for (int e = 0; e < PX; ++e)
                    if (e < n) d[e] = a.norm[v[e][c]];
            }
        }
    }
    uint8_t* bytes = OP == OP_STREAM_U8 ? a.u8 : static_cast<uint8_t*>(a.dst);
    if (bytes == nullptr) return;
    const int C = OP == OP_STREAM_U8 ? 3 : a.C;
    bytes += out_px * C;
    if (WIDE && C == 3) {
        u32x3 o;
        o.x = (uint32_t)v[0][0] | ((uint32_t)v[0][1] << 8) | ((uint32_t)v[0][2] << 16) | ((uint32_t)v[1][0] << 24);
        o.y = (uint32_t)v[1][1] | ((uint32_t)v[1][2] << 8) | ((uint32_t)v[2][0] << 16) | ((uint32_t)v[2][1] << 24);
        o.z = (uint32_t)v[2][2] | ((uint32_t)v[3][0] << 8) | ((uint32_t)v[3][1] << 16) | ((uint32_t)v[3][2] << 24);
        *reinterpret_cast<u32x3*>(bytes) = o;
    } else if (WIDE) {
        *reinterpret_cast<uint32_t*>(bytes) = (uint32_t)v[0][0] | ((uint32_t)v[1][0] << 8) | ((uint32_t)v[2][0] << 16) | ((uint32_t)v[3][0] << 24);
    } else {
#pragma unroll
        for (int e = 0; e < PX; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (e < n && c < C) bytes[e * C + c] = (uint8_t)v[e][c];
    }
}

template <int OP>
int launch(const FramesArgs& a, int T, bool wide, void* stream, const char* what) {
    const dim3 grid((unsigned)((a.W + BLOCK * PX - 1) / (BLOCK * PX)), (unsigned)a.H, (unsigned)T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL((frames_kernel<OP, true>), grid, dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((frames_kernel<OP, false>), grid, dim3(BLOCK), 0, s, a);
    return mudg_check_launch(what);
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int mudg_resize_u8(const uint8_t* src, uint8_t* dst, int T, int H0, int W0, int C, int H, int W, int mode, int palette,
                              const int32_t* xtab, const int32_t* ytab, void* stream) {
    MUDG_REQUIRE(src && dst && xtab && ytab, "mudg_resize_u8: null pointer");
    FRAMES_REQUIRE_SIZES("mudg_resize_u8");
    MUDG_REQUIRE(mode == MUDG_RESIZE_LINEAR || mode == MUDG_RESIZE_NEAREST, "mudg_resize_u8: mode %d (0 linear, 1 nearest)", mode);
    MUDG_REQUIRE(C == 1 || C == 3, "mudg_resize_u8: %d channels (one or three)", C);
    MUDG_REQUIRE(!palette || (C == 3 && mode == MUDG_RESIZE_LINEAR), "mudg_resize_u8: the label palette gives three channels under the linear rule");
    MUDG_REQUIRE(aligned16(xtab) && aligned16(ytab), "mudg_resize_u8: the tables are 16-byte entries, 16-byte aligned");
    FramesArgs a = {};
    a.src = src; a.xt = reinterpret_cast<const Tap*>(xtab); a.yt = reinterpret_cast<const Tap*>(ytab); a.dst = dst;
    a.H0 = H0; a.W0 = W0; a.CS = palette ? 1 : C; a.C = C; a.H = H; a.W = W; a.palette = palette ? 1 : 0;
    const bool wide = (W & 3) == 0 && aligned4(dst);
    return mode == MUDG_RESIZE_LINEAR ? launch<OP_U8_LINEAR>(a, T, wide, stream, "mudg_resize_u8")
                                      : launch<OP_U8_NEAREST>(a, T, wide, stream, "mudg_resize_u8");
}

extern "C" int mudg_resize_f32(const float* src, float* dst, int T, int H0, int W0, int H, int W, const int32_t* xtab,
                               const int32_t* ytab, void* stream) {
    MUDG_REQUIRE(src && dst && xtab && ytab, "mudg_resize_f32: null pointer");
    FRAMES_REQUIRE_SIZES("mudg_resize_f32");
    MUDG_REQUIRE(aligned16(xtab) && aligned16(ytab), "mudg_resize_f32: the tables are 16-byte entries, 16-byte aligned");
    FramesArgs a = {};
    a.src = src; a.xt = reinterpret_cast<const Tap*>(xtab); a.yt = reinterpret_cast<const Tap*>(ytab); a.dst = dst;
    a.H0 = H0; a.W0 = W0; a.CS = 1; a.C = 1; a.H = H; a.W = W;
    return launch<OP_F32>(a, T, (W & 3) == 0 && aligned16(dst), stream, "mudg_resize_f32");
}

extern "C" int mudg_dense_stream(int kind, const void* src, int T, int H0, int W0, int H, int W, const int32_t* xtab,
                                 const int32_t* ytab, const float* norm, float* dst, int64_t stream_stride, int64_t channel_stride,
                                 int64_t frame_stride, int slab, int frame0, uint8_t* u8_out, void* stream) {
    MUDG_REQUIRE(src && dst && xtab && ytab, "mudg_dense_stream: null pointer");
    MUDG_REQUIRE(kind == MUDG_STREAM_COLOUR || kind == MUDG_STREAM_SEMANTIC || kind == MUDG_STREAM_DEPTH,
                 "mudg_dense_stream: kind %d (0 colour, 1 semantic, 2 depth)", kind);
    FRAMES_REQUIRE_SIZES("mudg_dense_stream");
    MUDG_REQUIRE(aligned16(xtab) && aligned16(ytab), "mudg_dense_stream: the tables are 16-byte entries, 16-byte aligned");
    MUDG_REQUIRE(kind == MUDG_STREAM_DEPTH ? u8_out == nullptr : norm != nullptr,
                 "mudg_dense_stream: a stream of bytes needs the normalisation table, the depth stream has no uint8 output");
    MUDG_REQUIRE(frame_stride >= (int64_t)H * W && channel_stride > 0 && stream_stride >= 0 && slab >= 0 && frame0 >= 0,
                 "mudg_dense_stream: strides %lld / %lld / %lld at stream %d, frame %d (frames at least H W = %lld floats apart)",
                 (long long)stream_stride, (long long)channel_stride, (long long)frame_stride, slab, frame0, (long long)H * W);
    MUDG_REQUIRE(aligned4(dst), "mudg_dense_stream: the destination is fp32");
    FramesArgs a = {};
    a.src = src; a.xt = reinterpret_cast<const Tap*>(xtab); a.yt = reinterpret_cast<const Tap*>(ytab); a.norm = norm;
    a.dst = dst + slab * stream_stride + frame0 * frame_stride; a.u8 = u8_out;
    a.H0 = H0; a.W0 = W0; a.CS = kind == MUDG_STREAM_COLOUR ? 3 : 1; a.C = 3; a.H = H; a.W = W; a.palette = kind == MUDG_STREAM_SEMANTIC;
    a.cs = channel_stride; a.fs = frame_stride;
    const bool wide = (W & 3) == 0 && aligned16(a.dst) && (channel_stride & 3) == 0 && (frame_stride & 3) == 0 && aligned4(u8_out);
    return kind == MUDG_STREAM_DEPTH ? launch<OP_STREAM_DEPTH>(a, T, wide, stream, "mudg_dense_stream")
                                     : launch<OP_STREAM_U8>(a, T, wide, stream, "mudg_dense_stream");
}
