// splat.hip — the sparse conditions: a fused point cloud drawn into the camera at virtual poses.
//   splat_points   a lane owns a point (16 bytes: x, y, z fp32 and the colour in the fourth word): projected into every pose of the
//                  frame, one 64-bit atomic minimum of (bits(zc) << 32 | index) per covered pixel              generate_sparse.py:153-175
//   splat_resolve  a lane owns one or four pixels: key -> depth and the winner's colour word; the key image is cleared for the next frame
//   splat_compose  the 13 x 13 dilation of the object mask through LDS, the background / object select and the condition arithmetic,
//                  written into (3, T, H, W) tensors at frame t                       generate_sparse.py:208-223, data_tools.py:53-54, 93-94
// Everything is fp32 in a fixed order with correctly rounded operations, and the depth test is an integer minimum: the images do not
// depend on the order in which the points arrive and are bit-equal to the numpy definition in tests/splat_reference.py.
#include "splat_shared.h"

namespace {

constexpr uint64_t EMPTY = SPLAT_EMPTY;

// OBJ = false: one matrix per pose, the same for every lane (uniform addresses: the matrices sit in scalar registers).
// OBJ = true: matrix (pose, id[point]) of `nmat` per pose.  STATS: count covered pixels and issued atomics (tools only).
template <bool OBJ, bool STATS>
__global__ __launch_bounds__(256) void splat_points_kernel(const u32x4* __restrict__ pts, const int32_t* __restrict__ ids,
                                                            const float* __restrict__ mats, unsigned long long* __restrict__ keys,
                                                            unsigned long long* __restrict__ stats, int64_t n, int P, int nmat,
                                                            int H, int W, SplatCam cam, int early_reject) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned covered = 0, issued = 0;
    if (idx < n) {
        const u32x4 q = pts[idx];                                          // one 16-byte load
        const float x = __uint_as_float(q.x), y = __uint_as_float(q.y), z = __uint_as_float(q.z);
        int id = 0;
        if (OBJ) { id = ids[idx]; id = id < 0 ? 0 : (id >= nmat ? nmat - 1 : id); }
        const int64_t plane = (int64_t)H * W;
        for (int p = 0; p < P; ++p) {
            const float* m = mats + ((int64_t)p * nmat + id) * 12;
            float zc, u, v;
            int i0, i1, j0, j1;
            if (!splat_project(m, x, y, z, cam, H, W, zc, u, v, i0, i1, j0, j1)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | (unsigned long long)(uint32_t)idx;
            unsigned long long* img = keys + p * plane;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) {
                    unsigned long long* k = img + (int64_t)j * W + i;          // 0 <= j < H, 0 <= i < W by cover()
                    if (STATS) ++covered;
                    // Most points of a dense cloud are hidden: a load that finds a smaller key saves the atomic.  Keys only ever
                    // decrease, so a stale value can only fail to skip.
                    if (early_reject && __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;
                    if (STATS) ++issued;
                    __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    }
    if (STATS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { covered += __shfl_xor(covered, o, 64); issued += __shfl_xor(issued, o, 64); }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(stats, (unsigned long long)covered);
            atomicAdd(stats + 1, (unsigned long long)issued);
        }
    }
}

__device__ __forceinline__ void resolve_one(unsigned long long key, const uint32_t* __restrict__ pts, int64_t n, float& depth, uint32_t& colour) {
    depth = 0.0f;
    colour = 0u;
    if (key != EMPTY && (int64_t)(uint32_t)key < n) {                     // an index beyond the cloud: not this cloud's key image
        depth = __uint_as_float((uint32_t)(key >> 32));
        colour = pts[4 * (int64_t)(uint32_t)key + 3] & 0x00ffffffu;
    }
}

// PX = 4: a lane owns four pixels: two 16-byte key loads, two 16-byte key stores (the clear), one 16-byte store each of depth and colour.
template <int PX>
__global__ __launch_bounds__(256) void splat_resolve_kernel(unsigned long long* __restrict__ keys, const uint32_t* __restrict__ pts,
                                                             float* __restrict__ depth, uint32_t* __restrict__ colour, int64_t n, int64_t total) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PX;
    if (i >= total) return;
    if (PX == 4) {
        const u32x4 a = ld16(keys + i), b = ld16(keys + i + 2);
        const unsigned long long k[4] = {((unsigned long long)a.y << 32) | a.x, ((unsigned long long)a.w << 32) | a.z,
                                         ((unsigned long long)b.y << 32) | b.x, ((unsigned long long)b.w << 32) | b.z};
        f32x4 d;
        u32x4 c;
#pragma unroll
        for (int e = 0; e < 4; ++e) { float de; uint32_t ce; resolve_one(k[e], pts, n, de, ce); d[e] = de; c[e] = ce; }
        *reinterpret_cast<f32x4*>(depth + i) = d;
        st16(colour + i, c);
        const u32x4 ones = {~0u, ~0u, ~0u, ~0u};
        st16(keys + i, ones);
        st16(keys + i + 2, ones);
    } else {
        float de; uint32_t ce;
        resolve_one(keys[i], pts, n, de, ce);
        depth[i] = de;
        colour[i] = ce;
        keys[i] = EMPTY;
    }
}

// ---- compose: a 64 x 16 tile of one pose per workgroup --------------------------------------------------------------------------
constexpr int TW = 64, TH = 16, HALO = 6;

__device__ __forceinline__ float cond_colour(uint32_t byte) {                  // (c / 255 - 0.5) * 2
    return __fmul_rn(__fsub_rn(__fdiv_rn((float)byte, 255.0f), 0.5f), 2.0f);
}
__device__ __forceinline__ float cond_depth(float d) {                         // (clamp(d, 0, 100) / 100 - 0.5) * 2
    return __fmul_rn(__fsub_rn(__fdiv_rn(fminf(fmaxf(d, 0.0f), 100.0f), 100.0f), 0.5f), 2.0f);
}

__global__ __launch_bounds__(256) void splat_compose_kernel(const uint32_t* __restrict__ bg_c, const float* __restrict__ bg_d,
                                                             const uint32_t* __restrict__ ob_c, const float* __restrict__ ob_d,
                                                             float* __restrict__ sparse, float* __restrict__ sdepth, int64_t pose_stride,
                                                             int T, int t, int H, int W, uint8_t* __restrict__ rgb_out,
                                                             float* __restrict__ depth_out, uint8_t* __restrict__ mask_out) {
    __shared__ uint8_t set[TH + 2 * HALO][TW + 2 * HALO];          // all(obj_rgb > 0), 0 outside the image
    __shared__ uint8_t rows[TH + 2 * HALO][TW];                    // after the row pass: any of 13 along the width
    const int p = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t plane = (int64_t)H * W;
    const uint32_t* oc = ob_c ? ob_c + p * plane : nullptr;
    if (oc) {                                                       // uniform across the grid
        for (int e = threadIdx.x; e < (TH + 2 * HALO) * (TW + 2 * HALO); e += 256) {
            const int r = e / (TW + 2 * HALO), c = e % (TW + 2 * HALO);
            const int y = y0 + r - HALO, x = x0 + c - HALO;
            uint8_t f = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const uint32_t w = oc[(int64_t)y * W + x];
                f = (w & 0xffu) && (w & 0xff00u) && (w & 0xff0000u);
            }
            set[r][c] = f;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < (TH + 2 * HALO) * TW; e += 256) {
            const int r = e / TW, c = e % TW;
            uint8_t f = 0;
#pragma unroll
            for (int k = 0; k <= 2 * HALO; ++k) f |= set[r][c + k];
            rows[r][c] = f;
        }
        __syncthreads();
    }
    const int64_t tplane = (int64_t)T * plane;                      // one channel of one pose
    for (int e = threadIdx.x; e < TH * TW; e += 256) {
        const int r = e / TW, c = e % TW;
        const int y = y0 + r, x = x0 + c;
        if (y >= H || x >= W) continue;
        uint8_t m = 0;
        if (oc) {
#pragma unroll
            for (int k = 0; k <= 2 * HALO; ++k) m |= rows[r + k][c];
        }
        const int64_t pix = (int64_t)y * W + x, src = p * plane + pix;
        const uint32_t w = m ? oc[pix] : bg_c[src];
        const float d = m ? ob_d[src] : bg_d[src];
        const int64_t dst = p * pose_stride + (int64_t)t * plane + pix;
        const float cd = cond_depth(d);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            sparse[dst + ch * tplane] = cond_colour((w >> (8 * ch)) & 0xffu);
            sdepth[dst + ch * tplane] = cd;
        }
        if (rgb_out) {
            rgb_out[3 * src] = (uint8_t)w; rgb_out[3 * src + 1] = (uint8_t)(w >> 8); rgb_out[3 * src + 2] = (uint8_t)(w >> 16);
        }
        if (depth_out) depth_out[src] = d;
        if (mask_out) mask_out[src] = m;
    }
}

}  // namespace

extern "C" int mudg_splat_points(const void* points, const int32_t* ids, int64_t n, const float* mats, int poses, int nmat,
                                 uint64_t* keys, int H, int W, float fx, float fy, float cx, float cy, float znear, float zfar,
                                 float point_size, int flags, uint64_t* stats, void* stream) {
    MUDG_REQUIRE(points && mats && keys && n > 0 && poses > 0 && nmat > 0 && H > 0 && W > 0, "mudg_splat_points: bad arguments");
    MUDG_REQUIRE(n <= 0xffffffffLL, "mudg_splat_points: %lld points (the key holds a 32-bit index)", (long long)n);
    MUDG_REQUIRE(aligned16(points) && (reinterpret_cast<uintptr_t>(keys) & 7u) == 0, "mudg_splat_points: unaligned points or keys");
    MUDG_REQUIRE(ids || nmat == 1, "mudg_splat_points: %d matrices per pose need per-point ids", nmat);
    MUDG_REQUIRE(point_size > 0.0f && point_size <= (float)MAX_SPRITE - 1.0f, "mudg_splat_points: point size %g (0 < size <= %d)", (double)point_size, MAX_SPRITE - 1);
    MUDG_REQUIRE(znear > 0.0f && zfar > znear, "mudg_splat_points: need 0 < znear < zfar (positive depths order like their bits)");
    MUDG_REQUIRE((int64_t)H * W < (1LL << 31) && H < (1 << 23) && W < (1 << 23), "mudg_splat_points: image too large");
    const SplatCam cam = {fx, fy, cx, cy, znear, zfar, point_size * 0.5f};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
    const u32x4* pts = reinterpret_cast<const u32x4*>(points);
    const int reject = (flags & MUDG_SPLAT_NO_EARLY_REJECT) ? 0 : 1;
    if (ids) {
        if (st) hipLaunchKernelGGL((splat_points_kernel<true, true>), grid, block, 0, s, pts, ids, mats, k, st, n, poses, nmat, H, W, cam, reject);
        else hipLaunchKernelGGL((splat_points_kernel<true, false>), grid, block, 0, s, pts, ids, mats, k, st, n, poses, nmat, H, W, cam, reject);
    } else {
        if (st) hipLaunchKernelGGL((splat_points_kernel<false, true>), grid, block, 0, s, pts, ids, mats, k, st, n, poses, nmat, H, W, cam, reject);
        else hipLaunchKernelGGL((splat_points_kernel<false, false>), grid, block, 0, s, pts, ids, mats, k, st, n, poses, nmat, H, W, cam, reject);
    }
    return mudg_check_launch("mudg_splat_points");
}

extern "C" int mudg_splat_resolve(uint64_t* keys, const void* points, int64_t n, float* depth, uint32_t* colour, int64_t pixels, void* stream) {
    MUDG_REQUIRE(keys && points && depth && colour && n > 0 && pixels > 0, "mudg_splat_resolve: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
    const uint32_t* pts = reinterpret_cast<const uint32_t*>(points);
    const bool wide = (pixels & 3) == 0 && aligned16(keys) && aligned16(depth) && aligned16(colour);
    const int64_t lanes = wide ? pixels / 4 : pixels;
    MUDG_REQUIRE((lanes + 255) / 256 <= 0x7fffffffLL, "mudg_splat_resolve: image too large");
    if (wide) hipLaunchKernelGGL(splat_resolve_kernel<4>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, k, pts, depth, colour, n, pixels);
    else hipLaunchKernelGGL(splat_resolve_kernel<1>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, k, pts, depth, colour, n, pixels);
    return mudg_check_launch("mudg_splat_resolve");
}

extern "C" int mudg_splat_compose(const uint32_t* bg_colour, const float* bg_depth, const uint32_t* obj_colour, const float* obj_depth,
                                  float* sparse_frames, float* sparse_depth, int64_t pose_stride, int poses, int T, int t, int H, int W,
                                  uint8_t* rgb_out, float* depth_out, uint8_t* mask_out, void* stream) {
    MUDG_REQUIRE(bg_colour && bg_depth && sparse_frames && sparse_depth && poses > 0 && H > 0 && W > 0, "mudg_splat_compose: bad arguments");
    MUDG_REQUIRE((obj_colour == nullptr) == (obj_depth == nullptr), "mudg_splat_compose: object colour and depth come together");
    MUDG_REQUIRE(T > 0 && t >= 0 && t < T, "mudg_splat_compose: frame %d of %d", t, T);
    MUDG_REQUIRE(pose_stride >= (int64_t)3 * T * H * W, "mudg_splat_compose: poses overlap (stride %lld)", (long long)pose_stride);
    MUDG_REQUIRE(poses <= 65535 && (H + TH - 1) / TH <= 65535, "mudg_splat_compose: grid too large");
    const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)poses);
    hipLaunchKernelGGL(splat_compose_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), bg_colour, bg_depth, obj_colour,
                       obj_depth, sparse_frames, sparse_depth, pose_stride, T, t, H, W, rgb_out, depth_out, mask_out);
    return mudg_check_launch("mudg_splat_compose");
}
