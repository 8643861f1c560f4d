// gaussians.hip — a cloud drawn as 3D Gaussians: the forward half of a tile-binned splat renderer.
//   gauss_project  a lane owns a Gaussian (a packed 16-byte point of §12, six covariance entries, an opacity, a matrix id), read once
//                  and projected into every view of the call: image position, EWA conic, depth, tile rectangle, tile count
//   gauss_keys     a lane owns a (view, Gaussian): one (tile << 32 | bits(zc), index) entry per tile of its rectangle, at the offsets
//                  of an exclusive scan of the counts; the host sorts the keys (torch.sort, stable)
//   gauss_ranges   a lane owns a sorted entry: where the tile changes, the [start, end) of that tile; plain stores
//   gauss_blend    a workgroup owns a 16 x 16 tile of one view, a lane a pixel: the tile's entries through LDS in batches of 256,
//                  front-to-back alpha blending until every pixel of the tile is opaque
// Everything is fp32, each operation a single correctly rounded one in the order DESIGN.md §23 writes it (the library is built without
// contraction, and the intrinsics say so again); the exponential is a fixed polynomial, so the images are bit-equal to the numpy
// definition in tests/gaussians_reference.py.  No atomics on global memory (the counting barrier of the blend adds in LDS): a repeat run
// gives the same bits.  No MFMA operand is touched: the same code in every library build.
#include "gauss_shared.h"

namespace {

__global__ __launch_bounds__(256) void gauss_project_kernel(const u32x4* __restrict__ pts, const float* __restrict__ cov,
                                                             const float* __restrict__ opacity, const int32_t* __restrict__ ids,
                                                             const float* __restrict__ mats, int64_t n, int V, int nmat, int H, int W,
                                                             GaussCam cam, f32x2* __restrict__ uv, f32x4* __restrict__ conic,
                                                             float* __restrict__ depth, u32x4* __restrict__ rect, int32_t* __restrict__ count) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const GaussPoint g = load_gaussian(pts, cov, ids, nmat, idx);
    const float op = opacity[idx];
    const GaussGrid grid(H, W);
    const float limx = gauss_limit(W, cam.fx), limy = gauss_limit(H, cam.fy);
    for (int view = 0; view < V; ++view) {
        const int64_t o = (int64_t)view * n + idx;
        f32x2 out_uv = {0.0f, 0.0f};
        f32x4 out_conic = {0.0f, 0.0f, 0.0f, 0.0f};
        float out_z = 0.0f;
        u32x4 out_rect = {0u, 0u, 0u, 0u};
        int out_count = 0;
        GaussView w;
        if (gauss_view(mats + ((int64_t)view * nmat + g.id) * 12, g, cam, limx, limy, w) && w.det > 0.0f && w.det < INFINITY) {
            const float mid = mul(0.5f, add(w.a, w.c));
            const float lam = add(mid, __fsqrt_rn(fmaxf(0.1f, sub(mul(mid, mid), w.det))));
            const float rad = ceilf(mul(3.0f, __fsqrt_rn(lam)));
            if (rad <= MAX_RADIUS && op >= MIN_ALPHA && op < INFINITY) {                     // false for what is not a number
                const float fTX = (float)grid.TX, fTY = (float)grid.TY;
                const int x0 = (int)clampf(floorf(dvd(sub(w.u, rad), 16.0f)), 0.0f, fTX);
                const int x1 = (int)clampf(add(floorf(dvd(add(w.u, rad), 16.0f)), 1.0f), 0.0f, fTX);
                const int y0 = (int)clampf(floorf(dvd(sub(w.v, rad), 16.0f)), 0.0f, fTY);
                const int y1 = (int)clampf(add(floorf(dvd(add(w.v, rad), 16.0f)), 1.0f), 0.0f, fTY);
                const int tiles = (x1 - x0) * (y1 - y0);                                      // at most TX TY < 2^31
                if (tiles > 0) {
                    out_uv.x = w.u; out_uv.y = w.v;
                    out_conic.x = dvd(w.c, w.det); out_conic.y = -dvd(w.b, w.det); out_conic.z = dvd(w.a, w.det); out_conic.w = op;
                    out_z = w.zc;
                    out_rect.x = (uint32_t)x0; out_rect.y = (uint32_t)x1; out_rect.z = (uint32_t)y0; out_rect.w = (uint32_t)y1;
                    out_count = tiles;
                }
            }
        }
        uv[o] = out_uv;
        conic[o] = out_conic;
        depth[o] = out_z;
        rect[o] = out_rect;
        count[o] = out_count;
    }
}

// Entry offsets[o] + k is tile k of the rectangle in row-major order.  A rectangle that is not inside the tile grid, a count that is not
// the rectangle's or an offset that leaves [0, E) writes nothing: no address depends on a value that was not checked.
__global__ __launch_bounds__(256) void gauss_keys_kernel(const float* __restrict__ depth, const u32x4* __restrict__ rect,
                                                          const int32_t* __restrict__ count, const int64_t* __restrict__ offsets, int64_t n,
                                                          int64_t total, int TX, int TY, int64_t E, long long* __restrict__ keys,
                                                          int32_t* __restrict__ values) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int c = count[o];
    if (c <= 0) return;
    const u32x4 r = rect[o];
    const int x0 = (int)r.x, x1 = (int)r.y, y0 = (int)r.z, y1 = (int)r.w;
    if (x0 < 0 || x1 > TX || x0 >= x1 || y0 < 0 || y1 > TY || y0 >= y1) return;
    if ((int64_t)(x1 - x0) * (y1 - y0) != c) return;
    const int64_t at = offsets[o];
    if (at < 0 || at > E - c) return;
    const int64_t view = o / n;
    const int32_t index = (int32_t)(o - view * n);
    const long long first = view * ((long long)TX * TY);
    const long long low = (long long)__float_as_uint(depth[o]);
    int64_t e = at;
    for (int ty = y0; ty < y1; ++ty)
        for (int tx = x0; tx < x1; ++tx, ++e) {
            keys[e] = ((first + (long long)ty * TX + tx) << 32) | low;
            values[e] = index;
        }
}

__global__ __launch_bounds__(256) void gauss_ranges_kernel(const long long* __restrict__ keys, int64_t E, int64_t tiles,
                                                            int32_t* __restrict__ ranges) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const long long tile = keys[e] >> 32;
    if (tile < 0 || tile >= tiles) return;                                  // not a key of this call
    if (e == 0 || (keys[e - 1] >> 32) != tile) ranges[2 * tile] = (int32_t)e;
    if (e == E - 1 || (keys[e + 1] >> 32) != tile) ranges[2 * tile + 1] = (int32_t)(e + 1);
}

// An entry in LDS is 32 bytes: stage_batch's two words with the colour word in the free slot.  walked (tools; may be NULL): the
// entries this workgroup staged before it left.
__global__ __launch_bounds__(256) void gauss_blend_kernel(const uint32_t* __restrict__ pts, const f32x2* __restrict__ uv,
                                                           const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                           const int32_t* __restrict__ values, const int32_t* __restrict__ ranges, int64_t n,
                                                           int64_t E, int TX, int NT, int H, int W, float* __restrict__ rgb,
                                                           float* __restrict__ depth_out, float* __restrict__ alpha_out,
                                                           int32_t* __restrict__ walked) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    const GaussTile tile = gauss_tile(blockIdx.x, ranges, E, TX, NT, H, W);
    GaussPixel acc;
    const int64_t staged = blend_forward(uv, conic, depth, values, n, tile, ByteColour{pts}, geom, look, acc);
    if (walked && threadIdx.x == 0) walked[blockIdx.x] = (int32_t)staged;
    if (tile.inside) store_images(tile, H, W, acc, rgb, depth_out, alpha_out);
}

}  // namespace

extern "C" int mudg_gauss_project(const void* points, const float* cov, const float* opacity, const int32_t* ids, int64_t n,
                                  const float* mats, int V, int nmat, int H, int W, float fx, float fy, float cx, float cy, float znear,
                                  float zfar, float* uv, float* conic, float* depth, int32_t* rect, int32_t* count, void* stream) {
    MUDG_REQUIRE(points && cov && opacity && mats && uv && conic && depth && rect && count, "mudg_gauss_project: null argument");
    MUDG_REQUIRE(aligned16(points), "mudg_gauss_project: unaligned points");
    MUDG_REQUIRE(aligned16(conic) && aligned16(rect) && aligned8(uv), "mudg_gauss_project: unaligned outputs");
    MUDG_REQUIRE(nmat > 0, "mudg_gauss_project: %d matrices per view", nmat);
    if (const int e = check_views("mudg_gauss_project", n, V, H, W)) return e;
    MUDG_REQUIRE(ids || nmat == 1, "mudg_gauss_project: %d matrices per view need per-point ids", nmat);
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_project: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    if (const int e = check_camera("mudg_gauss_project", fx, fy, cx, cy, znear, zfar, " (positive depths order like their bits)")) return e;
    const GaussCam cam = {fx, fy, cx, cy, znear, zfar};
    hipLaunchKernelGGL(gauss_project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(points), cov, opacity, ids, mats, n, V, nmat, H, W, cam, reinterpret_cast<f32x2*>(uv),
                       reinterpret_cast<f32x4*>(conic), depth, reinterpret_cast<u32x4*>(rect), count);
    return mudg_check_launch("mudg_gauss_project");
}

extern "C" int mudg_gauss_keys(const float* depth, const int32_t* rect, const int32_t* count, const int64_t* offsets, int64_t n, int V,
                               int H, int W, int64_t E, int64_t* keys, int32_t* values, void* stream) {
    MUDG_REQUIRE(depth && rect && count && offsets && keys && values, "mudg_gauss_keys: null argument");
    MUDG_REQUIRE(aligned16(rect), "mudg_gauss_keys: unaligned rectangles");
    if (const int e = check_views("mudg_gauss_keys", n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_keys: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const int64_t total = (int64_t)V * n;
    const GaussGrid grid(H, W);
    MUDG_REQUIRE(grid_ok(total), "mudg_gauss_keys: %lld (view, Gaussian) pairs are more workgroups than a grid holds", (long long)total);
    hipLaunchKernelGGL(gauss_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth,
                       reinterpret_cast<const u32x4*>(rect), count, offsets, n, total, grid.TX, grid.TY, E,
                       reinterpret_cast<long long*>(keys), values);
    return mudg_check_launch("mudg_gauss_keys");
}

extern "C" int mudg_gauss_ranges(const int64_t* keys_sorted, int64_t E, int64_t tiles, int32_t* ranges, void* stream) {
    MUDG_REQUIRE(keys_sorted && ranges, "mudg_gauss_ranges: null argument");
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_ranges: %lld entries (1 .. 2^31 - 1)", (long long)E);
    MUDG_REQUIRE(tiles > 0 && tiles < (1LL << 31), "mudg_gauss_ranges: %lld tiles (V NT < 2^31)", (long long)tiles);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(ranges, 0, (size_t)tiles * 2 * sizeof(int32_t), s) != hipSuccess) return mudg_check_launch("mudg_gauss_ranges");
    hipLaunchKernelGGL(gauss_ranges_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const long long*>(keys_sorted), E,
                       tiles, ranges);
    return mudg_check_launch("mudg_gauss_ranges");
}

extern "C" int mudg_gauss_blend(const void* points, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                                const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb, float* depth_out,
                                float* alpha, int32_t* walked, void* stream) {
    MUDG_REQUIRE(points && uv && conic && depth && values_sorted && ranges && rgb && depth_out && alpha, "mudg_gauss_blend: null argument");
    MUDG_REQUIRE(aligned16(points), "mudg_gauss_blend: unaligned points");
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv), "mudg_gauss_blend: unaligned projections");
    if (const int e = check_views("mudg_gauss_blend", n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_blend: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const GaussGrid grid(H, W);
    hipLaunchKernelGGL(gauss_blend_kernel, dim3((unsigned)((int64_t)V * grid.NT)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t*>(points), reinterpret_cast<const f32x2*>(uv), reinterpret_cast<const f32x4*>(conic), depth,
                       values_sorted, ranges, n, E, grid.TX, grid.NT, H, W, rgb, depth_out, alpha, walked);
    return mudg_check_launch("mudg_gauss_blend");
}
