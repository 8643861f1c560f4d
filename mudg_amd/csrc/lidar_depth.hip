// lidar_depth.hip — LiDAR depth maps and their dense completion: the scene's own depth in metres.
//   lidar_splat_visible  a lane owns a candidate point of a frame's window (up to 8 segments of the per-frame sweeps, or the objects'
//                        cloud with its matrices): §12's projection, then the image-space occlusion test against the occluder keys
//                        that splat_points drew, then one 64-bit atomic minimum per covered pixel        pipeline_depth.py:63-152
//   lidar_depth_resolve  keys -> metres (the key's high word), 0 where nothing landed; the keys (and the occluder keys) are empty again
//   depth_complete       the morphological completion of a sparse map, five launches over a caller's scratch:
//                          close    32 x 32 tiles with a 9-pixel halo in LDS: invert, 13-pixel diamond, 5 x 5 close, 7 x 7 fill
//                          columns  a lane owns a column: the rows above its first value take that value
//                          rowmax   the 31-wide row maximum through LDS; colfill: the 31-high column maximum of it into the empties
//                          finish   32 x 32 tiles with a 4-pixel halo: 5 x 5 median (a selection network in registers), the
//                                   normalised 5 x 5 binomial blur in fp64, invert back, the sky, the source map
// Steps 1-6 and 8 of the completion select among their inputs or subtract once; the blur sums at most 25 exact fp64 products of less
// than 2^53 in all and divides once: no output depends on the tiling or on the order of execution.  The splat's depth test is an
// integer minimum.  Everything is bit-equal to the numpy definition in tests/lidar_depth_reference.py.
#include "depth_shared.h"
#include "splat_shared.h"

namespace {

constexpr int MAX_SEGMENTS = 8;
constexpr int MAX_REACH = 16;

struct Segments {
    int64_t offset[MAX_SEGMENTS];              // the segment's first point in the cloud
    int64_t start[MAX_SEGMENTS + 1];           // its first candidate number; start[count] = total
    int64_t total;
    int count;
};

__device__ __forceinline__ bool nearer(const unsigned long long* __restrict__ Z, int H, int W, int j, int i, float limit) {
    if (j < 0 || j >= H || i < 0 || i >= W) return false;
    const unsigned long long k = Z[(int64_t)j * W + i];
    return k != SPLAT_EMPTY && __uint_as_float((uint32_t)(k >> 32)) < limit;
}

template <bool OBJ>
__global__ __launch_bounds__(256) void lidar_splat_visible_kernel(const u32x4* __restrict__ pts, const int32_t* __restrict__ ids, const Segments seg,
                                                                   const float* __restrict__ mats, int nmat,
                                                                   const unsigned long long* __restrict__ Z, unsigned long long* __restrict__ keys,
                                                                   int H, int W, SplatCam cam, int reach, float keep, uint32_t index_base) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= seg.total) return;
    int s = 0;
    while (s + 1 < seg.count && idx >= seg.start[s + 1]) ++s;                 // at most 7 steps over scalar registers
    const int64_t at = seg.offset[s] + (idx - seg.start[s]);
    const u32x4 q = pts[at];
    int id = 0;
    if (OBJ) { id = ids[at]; id = id < 0 ? 0 : (id >= nmat ? nmat - 1 : id); }
    float zc, u, v;
    int i0, i1, j0, j1;
    if (!splat_project(mats + (int64_t)id * 12, __uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), cam, H, W, zc, u, v, i0, i1, j0, j1)) return;
    if (Z) {
        const int jh = (int)floorf(v), ih = (int)floorf(u);                   // |u|, |v| are within a sprite of the image: no overflow
        const float limit = __fmul_rn(zc, keep);
        const int dj[4] = {0, 1, 1, 1}, di[4] = {1, 0, 1, -1};
        bool hidden = false;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            bool plus = false, minus = false;
            for (int k = 1; k <= reach; ++k) {
                plus = plus || nearer(Z, H, W, jh + k * dj[d], ih + k * di[d], limit);
                minus = minus || nearer(Z, H, W, jh - k * dj[d], ih - k * di[d], limit);
            }
            hidden = hidden || (plus && minus);
        }
        if (hidden) return;
    }
    const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | (unsigned long long)(index_base + (uint32_t)idx);
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i)                                        // 0 <= j < H, 0 <= i < W by cover()
            __hip_atomic_fetch_min(keys + (int64_t)j * W + i, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void lidar_depth_resolve_kernel(unsigned long long* __restrict__ keys, unsigned long long* __restrict__ Z,
                                                                   float* __restrict__ depth, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const unsigned long long k = keys[i];
    depth[i] = k == SPLAT_EMPTY ? 0.0f : __uint_as_float((uint32_t)(k >> 32));
    keys[i] = SPLAT_EMPTY;
    if (Z) Z[i] = SPLAT_EMPTY;
}

// ---- completion ------------------------------------------------------------------------------------------------------------------
constexpr int TILE = 32;
constexpr int CLOSE_HALO = 9, CLOSE_SIDE = TILE + 2 * CLOSE_HALO;             // 2 (diamond) + 2 + 2 (close) + 3 (fill)
constexpr int FINISH_HALO = 4, FINISH_SIDE = TILE + 2 * FINISH_HALO, MEDIAN_SIDE = TILE + 4;
constexpr int REACH31 = 15;
constexpr float EMPTY_BELOW = 0.1f;

__device__ __forceinline__ bool filled(float x) { return x >= EMPTY_BELOW; }

// step 1: metres -> inverted depth, 0 where the pixel is empty (no return, not a number, or within 0.1 of max_depth or beyond)
__device__ __forceinline__ float inverted(float d, float M) {
    const float x = d > EMPTY_BELOW ? __fsub_rn(M, d) : 0.0f;
    return filled(x) ? x : 0.0f;
}

__global__ __launch_bounds__(256) void complete_close_kernel(const float* __restrict__ depth, float* __restrict__ x, uint8_t* __restrict__ stage,
                                                              int H, int W, float M) {
    __shared__ float a[CLOSE_SIDE][CLOSE_SIDE + 1], b[CLOSE_SIDE][CLOSE_SIDE + 1];
    const int64_t base = (int64_t)blockIdx.z * H * W;
    const int y0 = blockIdx.y * TILE - CLOSE_HALO, x0 = blockIdx.x * TILE - CLOSE_HALO;      // the image position of entry [0][0]
    auto inside = [&](int r, int c) { return y0 + r >= 0 && y0 + r < H && x0 + c >= 0 && x0 + c < W; };
    for (int e = threadIdx.x; e < CLOSE_SIDE * CLOSE_SIDE; e += 256) {
        const int r = e / CLOSE_SIDE, c = e % CLOSE_SIDE;
        a[r][c] = inside(r, c) ? inverted(depth[base + (int64_t)(y0 + r) * W + (x0 + c)], M) : 0.0f;
    }
    __syncthreads();
    {   // step 2: the diamond |dj| + |di| <= 2, a -> b on [2, SIDE - 2)
        constexpr int lo = 2, n = CLOSE_SIDE - 2 * lo;
        for (int e = threadIdx.x; e < n * n; e += 256) {
            const int r = lo + e / n, c = lo + e % n;
            float m = 0.0f;
            if (inside(r, c)) {
#pragma unroll
                for (int dj = -2; dj <= 2; ++dj)
#pragma unroll
                    for (int di = -2; di <= 2; ++di)
                        if ((dj < 0 ? -dj : dj) + (di < 0 ? -di : di) <= 2) m = fmaxf(m, a[r + dj][c + di]);
            }
            b[r][c] = m;
        }
    }
    __syncthreads();
    {   // step 3, the maximum over 5 x 5: b -> a on [4, SIDE - 4); what is outside the image holds 0, which is empty
        constexpr int lo = 4, n = CLOSE_SIDE - 2 * lo;
        for (int e = threadIdx.x; e < n * n; e += 256) {
            const int r = lo + e / n, c = lo + e % n;
            float m = 0.0f;
            if (inside(r, c)) {
#pragma unroll
                for (int dj = -2; dj <= 2; ++dj)
#pragma unroll
                    for (int di = -2; di <= 2; ++di) m = fmaxf(m, b[r + dj][c + di]);
            }
            a[r][c] = m;
        }
    }
    __syncthreads();
    {   // step 3, the minimum over 5 x 5: a -> b on [6, SIDE - 6); pixels outside the image do not take part
        constexpr int lo = 6, n = CLOSE_SIDE - 2 * lo;
        for (int e = threadIdx.x; e < n * n; e += 256) {
            const int r = lo + e / n, c = lo + e % n;
            float m = 0.0f;
            if (inside(r, c)) {
                m = a[r][c];
#pragma unroll
                for (int dj = -2; dj <= 2; ++dj)
#pragma unroll
                    for (int di = -2; di <= 2; ++di)
                        if (inside(r + dj, c + di)) m = fminf(m, a[r + dj][c + di]);
            }
            b[r][c] = m;
        }
    }
    __syncthreads();
    // step 4: an empty pixel takes the maximum over 7 x 7
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int r = CLOSE_HALO + e / TILE, c = CLOSE_HALO + e % TILE;
        if (!inside(r, c)) continue;
        float m = b[r][c];
        if (!filled(m)) {
#pragma unroll
            for (int dj = -3; dj <= 3; ++dj)
#pragma unroll
                for (int di = -3; di <= 3; ++di) m = fmaxf(m, b[r + dj][c + di]);
        }
        const int64_t at = base + (int64_t)(y0 + r) * W + (x0 + c);
        x[at] = m;
        stage[at] = filled(inverted(depth[at], M)) ? 1 : (filled(m) ? 2 : 0);
    }
}

// step 5, first half: a lane owns a column
__global__ __launch_bounds__(256) void complete_columns_kernel(float* __restrict__ x, int H, int W) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= W) return;
    float* col = x + (int64_t)blockIdx.y * H * W + c;
    int t = 0;
    while (t < H && !filled(col[(int64_t)t * W])) ++t;
    if (t == H) return;
    const float v = col[(int64_t)t * W];
    for (int r = 0; r < t; ++r) col[(int64_t)r * W] = v;
}

// step 5, the 31 x 31 maximum in two passes: blockIdx = (row segment, row, frame)
__global__ __launch_bounds__(256) void complete_rowmax_kernel(const float* __restrict__ x, float* __restrict__ rows, int H, int W) {
    __shared__ float s[256 + 2 * REACH31];
    const int c0 = blockIdx.x * 256;
    const int64_t line = ((int64_t)blockIdx.z * H + blockIdx.y) * W;
    for (int e = threadIdx.x; e < 256 + 2 * REACH31; e += 256) {
        const int c = c0 - REACH31 + e;
        s[e] = c >= 0 && c < W ? x[line + c] : 0.0f;
    }
    __syncthreads();
    const int c = c0 + threadIdx.x;
    if (c >= W) return;
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k <= 2 * REACH31; ++k) m = fmaxf(m, s[threadIdx.x + k]);
    rows[line + c] = m;
}

__global__ __launch_bounds__(256) void complete_colfill_kernel(float* __restrict__ x, const float* __restrict__ rows, int H, int W) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int64_t base = (int64_t)blockIdx.y * H * W;
    if (filled(x[base + p])) return;
    const int j = p / W, i = p - j * W;
    float m = 0.0f;
    for (int r = max(j - REACH31, 0); r <= min(j + REACH31, H - 1); ++r) m = fmaxf(m, rows[base + (int64_t)r * W + i]);
    x[base + p] = m;
}

__device__ __forceinline__ void order(float& lo, float& hi) { const float a = fminf(lo, hi), b = fmaxf(lo, hi); lo = a; hi = b; }

// The 13th smallest of 25: among any m = 14, 13, .. 4 of the values that are left, the smallest and the largest cannot be it (at least
// m - 1 >= half of what is left lie on one side of each); drop both, take the next value in.  Three are left: their middle.
__device__ __forceinline__ float median25(const float (&v)[25]) {
    float w[14];
#pragma unroll
    for (int e = 0; e < 14; ++e) w[e] = v[e];
#pragma unroll
    for (int m = 14; m >= 4; --m) {
#pragma unroll
        for (int e = 0; e + 1 < m; ++e) order(w[e], w[e + 1]);                // the largest to w[m - 1]
#pragma unroll
        for (int e = m - 2; e >= 1; --e) order(w[e - 1], w[e]);               // the smallest to w[0]
        w[0] = v[14 + (14 - m)];                                              // m = 14 .. 4 take v[14] .. v[24] in
    }
    // w[0], w[1], w[2] are what is left (w[3] was the largest of the last four)
    order(w[0], w[1]);
    return fminf(fmaxf(w[0], w[2]), w[1]);
}

__global__ __launch_bounds__(256) void complete_finish_kernel(const float* __restrict__ x, const uint8_t* __restrict__ stage,
                                                               const int64_t* __restrict__ labels, long long sky_label, int H, int W, float M,
                                                               float* __restrict__ out, uint8_t* __restrict__ source) {
    __shared__ float xs[FINISH_SIDE][FINISH_SIDE + 1], ms[MEDIAN_SIDE][MEDIAN_SIDE + 1];
    const int64_t base = (int64_t)blockIdx.z * H * W;
    const int ty = blockIdx.y * TILE, tx = blockIdx.x * TILE;
    for (int e = threadIdx.x; e < FINISH_SIDE * FINISH_SIDE; e += 256) {          // step 6 replicates the border
        const int r = e / FINISH_SIDE, c = e % FINISH_SIDE;
        const int y = min(max(ty - FINISH_HALO + r, 0), H - 1), xx = min(max(tx - FINISH_HALO + c, 0), W - 1);
        xs[r][c] = x[base + (int64_t)y * W + xx];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < MEDIAN_SIDE * MEDIAN_SIDE; e += 256) {
        const int r = e / MEDIAN_SIDE, c = e % MEDIAN_SIDE;
        const int y = ty - 2 + r, xx = tx - 2 + c;
        float m = 0.0f;
        if (y >= 0 && y < H && xx >= 0 && xx < W) {
            float v[25];
#pragma unroll
            for (int dj = 0; dj < 5; ++dj)
#pragma unroll
                for (int di = 0; di < 5; ++di) v[dj * 5 + di] = xs[r + dj][c + di];
            m = median25(v);
        }
        ms[r][c] = m;
    }
    __syncthreads();
    const double wt[5] = {1.0, 4.0, 6.0, 4.0, 1.0};
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int r = e / TILE, c = e % TILE;
        const int y = ty + r, xx = tx + c;
        if (y >= H || xx >= W) continue;
        float v = ms[r + 2][c + 2];
        if (filled(v)) {                                                      // step 7: over the filled pixels of the 5 x 5 that are in the image
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int dj = -2; dj <= 2; ++dj)
#pragma unroll
                for (int di = -2; di <= 2; ++di) {
                    const float n = ms[r + 2 + dj][c + 2 + di];
                    if (y + dj >= 0 && y + dj < H && xx + di >= 0 && xx + di < W && filled(n)) {
                        const double k = wt[dj + 2] * wt[di + 2];
                        num = __dadd_rn(num, __dmul_rn(k, (double)n));
                        den = __dadd_rn(den, k);
                    }
                }
            v = __double2float_rn(__ddiv_rn(num, den));
        }
        const int64_t at = base + (int64_t)y * W + xx;
        const bool sky = labels && labels[at] == sky_label;
        const bool has = filled(v);
        out[at] = sky ? M : (has ? __fsub_rn(M, v) : 0.0f);
        if (source) {
            const uint8_t s = stage[at];
            source[at] = sky ? 4 : (has ? (s ? s : 3) : 0);
        }
    }
}

inline int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline bool complete_shape_ok(int frames, int H, int W) { return shape_ok(frames, H, W) && H <= 65535; }

}  // namespace

extern "C" int mudg_lidar_splat_visible(const void* points, const int32_t* ids, const int64_t* segments, int nseg, const float* mats, int nmat,
                                        const uint64_t* occluder_keys, uint64_t* keys, int H, int W, float fx, float fy, float cx, float cy,
                                        float znear, float zfar, float point_size, int reach, float rel_keep, int64_t index_base, void* stream) {
    MUDG_REQUIRE(points && segments && mats && keys && nmat > 0, "mudg_lidar_splat_visible: bad arguments");
    MUDG_REQUIRE(nseg >= 1 && nseg <= MAX_SEGMENTS, "mudg_lidar_splat_visible: %d segments (1 .. %d)", nseg, MAX_SEGMENTS);
    MUDG_REQUIRE(aligned16(points) && (reinterpret_cast<uintptr_t>(keys) & 7u) == 0 && (reinterpret_cast<uintptr_t>(occluder_keys) & 7u) == 0,
                 "mudg_lidar_splat_visible: unaligned points or keys");
    MUDG_REQUIRE(ids || nmat == 1, "mudg_lidar_splat_visible: %d matrices need per-point ids", nmat);
    MUDG_REQUIRE(point_size > 0.0f && point_size <= (float)MAX_SPRITE - 1.0f, "mudg_lidar_splat_visible: point size %g (0 < size <= %d)", (double)point_size, MAX_SPRITE - 1);
    MUDG_REQUIRE(znear > 0.0f && zfar > znear, "mudg_lidar_splat_visible: need 0 < znear < zfar (positive depths order like their bits)");
    MUDG_REQUIRE(splat_args_ok(H, W), "mudg_lidar_splat_visible: image %d x %d", H, W);
    MUDG_REQUIRE(!occluder_keys || (reach >= 1 && reach <= MAX_REACH), "mudg_lidar_splat_visible: reach %d (1 .. %d)", reach, MAX_REACH);
    MUDG_REQUIRE(!occluder_keys || (rel_keep > 0.0f && rel_keep <= 1.0f), "mudg_lidar_splat_visible: 1 - rel_tol = %g (0 <= rel_tol < 1)", (double)rel_keep);
    Segments seg = {};
    seg.count = nseg;
    for (int s = 0; s < nseg; ++s) {
        MUDG_REQUIRE(segments[2 * s] >= 0 && segments[2 * s + 1] > 0, "mudg_lidar_splat_visible: segment %d is (%lld, %lld)", s, (long long)segments[2 * s], (long long)segments[2 * s + 1]);
        seg.offset[s] = segments[2 * s];
        seg.start[s + 1] = seg.start[s] + segments[2 * s + 1];
    }
    const int64_t n = seg.total = seg.start[nseg];
    MUDG_REQUIRE(index_base >= 0 && index_base + n <= 0x100000000LL, "mudg_lidar_splat_visible: %lld candidates from %lld (the key holds a 32-bit index)", (long long)n, (long long)index_base);
    const SplatCam cam = {fx, fy, cx, cy, znear, zfar, point_size * 0.5f};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const u32x4* pts = reinterpret_cast<const u32x4*>(points);
    const unsigned long long* Z = reinterpret_cast<const unsigned long long*>(occluder_keys);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
    if (ids) hipLaunchKernelGGL(lidar_splat_visible_kernel<true>, grid, block, 0, st, pts, ids, seg, mats, nmat, Z, k, H, W, cam, reach, rel_keep, (uint32_t)index_base);
    else hipLaunchKernelGGL(lidar_splat_visible_kernel<false>, grid, block, 0, st, pts, ids, seg, mats, nmat, Z, k, H, W, cam, reach, rel_keep, (uint32_t)index_base);
    return mudg_check_launch("mudg_lidar_splat_visible");
}

extern "C" int mudg_lidar_depth_resolve(uint64_t* keys, uint64_t* occluder_keys, float* depth, int64_t pixels, void* stream) {
    MUDG_REQUIRE(keys && depth && pixels > 0 && (pixels + 255) / 256 <= 0x7fffffffLL, "mudg_lidar_depth_resolve: bad arguments");
    MUDG_REQUIRE((reinterpret_cast<uintptr_t>(keys) & 7u) == 0 && (reinterpret_cast<uintptr_t>(occluder_keys) & 7u) == 0 && aligned4(depth),
                 "mudg_lidar_depth_resolve: unaligned keys or depth");
    hipLaunchKernelGGL(lidar_depth_resolve_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<unsigned long long*>(keys), reinterpret_cast<unsigned long long*>(occluder_keys), depth, pixels);
    return mudg_check_launch("mudg_lidar_depth_resolve");
}

extern "C" int64_t mudg_depth_complete_scratch(int frames, int H, int W) {
    if (!complete_shape_ok(frames, H, W)) return -1;
    const int64_t px = (int64_t)frames * H * W;
    return 2 * round16(4 * px) + round16(px);                                 // x, the row maxima, the stage bytes
}

extern "C" int mudg_depth_complete(const float* depth, const int64_t* labels, int64_t sky_label, int frames, int H, int W, float max_depth,
                                   int extrapolate, float* out, uint8_t* source, void* scratch, int64_t scratch_bytes, void* stream) {
    MUDG_REQUIRE(depth && out && scratch, "mudg_depth_complete: null argument");
    MUDG_REQUIRE(complete_shape_ok(frames, H, W), "mudg_depth_complete: %d frames of %d x %d (1 .. 65535 frames and rows, at most 2^24 pixels each)", frames, H, W);
    MUDG_REQUIRE(max_depth > EMPTY_BELOW && max_depth <= 65536.0f, "mudg_depth_complete: max_depth %g (0.1 < max_depth <= 65536: the blur's sums stay exact)", (double)max_depth);
    MUDG_REQUIRE(aligned4(depth) && aligned4(out) && aligned16(scratch), "mudg_depth_complete: unaligned depth, output or scratch");
    MUDG_REQUIRE(scratch_bytes >= mudg_depth_complete_scratch(frames, H, W), "mudg_depth_complete: %lld bytes of scratch, %lld needed",
                 (long long)scratch_bytes, (long long)mudg_depth_complete_scratch(frames, H, W));
    const int64_t px = (int64_t)frames * H * W;
    float* x = reinterpret_cast<float*>(scratch);
    float* rows = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + round16(4 * px));
    uint8_t* stage = reinterpret_cast<uint8_t*>(scratch) + 2 * round16(4 * px);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 tiles((unsigned)((W + TILE - 1) / TILE), (unsigned)((H + TILE - 1) / TILE), (unsigned)frames);
    hipLaunchKernelGGL(complete_close_kernel, tiles, dim3(256), 0, s, depth, x, stage, H, W, max_depth);
    if (extrapolate) {
        hipLaunchKernelGGL(complete_columns_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)frames), dim3(256), 0, s, x, H, W);
        hipLaunchKernelGGL(complete_rowmax_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)frames), dim3(256), 0, s, x, rows, H, W);
        hipLaunchKernelGGL(complete_colfill_kernel, frame_grid(frames, H * W, 1), dim3(256), 0, s, x, rows, H, W);
    }
    hipLaunchKernelGGL(complete_finish_kernel, tiles, dim3(256), 0, s, x, stage, labels, (long long)sky_label, H, W, max_depth, out, source);
    return mudg_check_launch("mudg_depth_complete");
}
