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
    const u32x4 q = pts[idx];                                              // one 16-byte load
    const float x = __uint_as_float(q.x), y = __uint_as_float(q.y), z = __uint_as_float(q.z);
    const float sxx = cov[6 * idx], sxy = cov[6 * idx + 1], sxz = cov[6 * idx + 2], syy = cov[6 * idx + 3], syz = cov[6 * idx + 4],
                szz = cov[6 * idx + 5];
    const float s[3][3] = {{sxx, sxy, sxz}, {sxy, syy, syz}, {sxz, syz, szz}};
    const float op = opacity[idx];
    int id = 0;
    if (ids) { id = ids[idx]; id = id < 0 ? 0 : (id >= nmat ? nmat - 1 : id); }
    const int TX = (W + TILE - 1) / TILE, TY = (H + TILE - 1) / TILE;
    const float limx = mul(1.3f, dvd(mul(0.5f, (float)W), cam.fx)), limy = mul(1.3f, dvd(mul(0.5f, (float)H), cam.fy));
    for (int view = 0; view < V; ++view) {
        const float* m = mats + ((int64_t)view * nmat + id) * 12;
        const int64_t o = (int64_t)view * n + idx;
        f32x2 out_uv = {0.0f, 0.0f};
        f32x4 out_conic = {0.0f, 0.0f, 0.0f, 0.0f};
        float out_z = 0.0f;
        u32x4 out_rect = {0u, 0u, 0u, 0u};
        int out_count = 0;
        const float xc = add(add(add(mul(m[0], x), mul(m[1], y)), mul(m[2], z)), m[3]);
        const float yc = add(add(add(mul(m[4], x), mul(m[5], y)), mul(m[6], z)), m[7]);
        const float zc = add(add(add(mul(m[8], x), mul(m[9], y)), mul(m[10], z)), m[11]);
        if (zc > cam.znear && zc < cam.zfar) {
            const float qx = dvd(xc, zc), qy = dvd(yc, zc);
            const float u = add(mul(cam.fx, qx), cam.cx), v = add(mul(cam.fy, qy), cam.cy);
            const float tx = mul(fminf(limx, fmaxf(-limx, qx)), zc), ty = mul(fminf(limy, fmaxf(-limy, qy)), zc);
            const float zz = mul(zc, zc);
            const float j00 = dvd(cam.fx, zc), j02 = -dvd(mul(cam.fx, tx), zz);
            const float j11 = dvd(cam.fy, zc), j12 = -dvd(mul(cam.fy, ty), zz);
            float t0[3], t1[3], v0[3], v1[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t0[k] = add(mul(j00, m[k]), mul(j02, m[8 + k]));
                t1[k] = add(mul(j11, m[4 + k]), mul(j12, m[8 + k]));
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v0[k] = add(add(mul(t0[0], s[0][k]), mul(t0[1], s[1][k])), mul(t0[2], s[2][k]));
                v1[k] = add(add(mul(t1[0], s[0][k]), mul(t1[1], s[1][k])), mul(t1[2], s[2][k]));
            }
            const float a = add(add(add(mul(v0[0], t0[0]), mul(v0[1], t0[1])), mul(v0[2], t0[2])), BLUR);
            const float b = add(add(mul(v0[0], t1[0]), mul(v0[1], t1[1])), mul(v0[2], t1[2]));
            const float c = add(add(add(mul(v1[0], t1[0]), mul(v1[1], t1[1])), mul(v1[2], t1[2])), BLUR);
            const float det = sub(mul(a, c), mul(b, b));
            if (det > 0.0f && det < INFINITY) {
                const float mid = mul(0.5f, add(a, c));
                const float lam = add(mid, __fsqrt_rn(fmaxf(0.1f, sub(mul(mid, mid), det))));
                const float rad = ceilf(mul(3.0f, __fsqrt_rn(lam)));
                if (rad <= MAX_RADIUS && op >= MIN_ALPHA && op < INFINITY) {                 // false for what is not a number
                    const float fTX = (float)TX, fTY = (float)TY;
                    const int x0 = (int)clampf(floorf(dvd(sub(u, rad), 16.0f)), 0.0f, fTX);
                    const int x1 = (int)clampf(add(floorf(dvd(add(u, rad), 16.0f)), 1.0f), 0.0f, fTX);
                    const int y0 = (int)clampf(floorf(dvd(sub(v, rad), 16.0f)), 0.0f, fTY);
                    const int y1 = (int)clampf(add(floorf(dvd(add(v, rad), 16.0f)), 1.0f), 0.0f, fTY);
                    const int tiles = (x1 - x0) * (y1 - y0);                                  // at most TX TY < 2^31
                    if (tiles > 0) {
                        out_uv.x = u; out_uv.y = v;
                        out_conic.x = dvd(c, det); out_conic.y = -dvd(b, det); out_conic.z = dvd(a, det); out_conic.w = op;
                        out_z = zc;
                        out_rect.x = (uint32_t)x0; out_rect.y = (uint32_t)x1; out_rect.z = (uint32_t)y0; out_rect.w = (uint32_t)y1;
                        out_count = tiles;
                    }
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

// An entry in LDS is 32 bytes: (u, v, A, B) and (C, opacity, colour word, zc).  A sorted value outside the cloud becomes an entry of
// opacity 0, which every pixel skips.  walked (tools; may be NULL): the entries this workgroup staged before it left.
__global__ __launch_bounds__(256) void gauss_blend_kernel(const uint32_t* __restrict__ pts, const f32x2* __restrict__ uv,
                                                           const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                           const int32_t* __restrict__ values, const int32_t* __restrict__ ranges, int64_t n,
                                                           int64_t E, int TX, int NT, int H, int W, float* __restrict__ rgb,
                                                           float* __restrict__ depth_out, float* __restrict__ alpha_out,
                                                           int32_t* __restrict__ walked) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    const int64_t t = blockIdx.x;
    const int64_t view = t / NT;
    const int tile = (int)(t - view * NT);
    const int i = (tile % TX) * TILE + (threadIdx.x & (TILE - 1)), j = (tile / TX) * TILE + (threadIdx.x >> 4);
    const bool inside = i < W && j < H;
    int64_t start = ranges[2 * t], end = ranges[2 * t + 1];
    if (start < 0 || end > E || start > end) start = end = 0;              // not a range of this call's entries
    const float px = add((float)i, 0.5f), py = add((float)j, 0.5f);
    float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, D = 0.0f;
    int done = inside ? 0 : 1;
    int64_t base = start;
    for (; base < end; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch has been read by every lane
        const int64_t e = base + threadIdx.x;
        f32x4 g0 = {0.0f, 0.0f, 0.0f, 0.0f}, g1 = {0.0f, 0.0f, 0.0f, 0.0f};
        if (e < end) {
            const int64_t g = values[e];
            if (g >= 0 && g < n) {
                const int64_t o = view * n + g;
                const f32x2 p = uv[o];
                const f32x4 k = conic[o];
                g0.x = p.x; g0.y = p.y; g0.z = k.x; g0.w = k.y;
                g1.x = k.z; g1.y = k.w; g1.z = __uint_as_float(pts[4 * g + 3] & 0x00ffffffu); g1.w = depth[o];
            }
        }
        geom[threadIdx.x] = g0;
        look[threadIdx.x] = g1;
        __syncthreads();
        const int m = (int)(end - base < BATCH ? end - base : BATCH);
        for (int k = 0; k < m && !done; ++k) {
            const f32x4 a = geom[k], b = look[k];
            const float dx = sub(a.x, px), dy = sub(a.y, py);
            const float q = add(mul(mul(a.z, dx), dx), mul(mul(b.x, dy), dy));
            const float p = sub(mul(-0.5f, q), mul(mul(a.w, dx), dy));
            if (p > 0.0f || p < MIN_POWER) continue;
            const float al = fminf(MAX_ALPHA, mul(b.y, gauss_exp(p)));
            if (al < MIN_ALPHA) continue;
            const float Tn = mul(T, sub(1.0f, al));
            if (Tn < MIN_T) { done = 1; break; }
            const float w = mul(al, T);
            const uint32_t word = __float_as_uint(b.z);
            c0 = add(c0, mul((float)(word & 0xffu), w));
            c1 = add(c1, mul((float)((word >> 8) & 0xffu), w));
            c2 = add(c2, mul((float)((word >> 16) & 0xffu), w));
            D = add(D, mul(b.w, w));
            T = Tn;
        }
    }
    if (walked && threadIdx.x == 0) walked[t] = (int32_t)((base < end ? base : end) - start);
    if (inside) {
        const int64_t plane = (int64_t)H * W, pix = (int64_t)j * W + i;
        float* out = rgb + view * 3 * plane + pix;
        out[0] = dvd(c0, 255.0f);
        out[plane] = dvd(c1, 255.0f);
        out[2 * plane] = dvd(c2, 255.0f);
        depth_out[view * plane + pix] = D;
        alpha_out[view * plane + pix] = sub(1.0f, T);
    }
}

}  // namespace

extern "C" int mudg_gauss_project(const void* points, const float* cov, const float* opacity, const int32_t* ids, int64_t n,
                                  const float* mats, int V, int nmat, int H, int W, float fx, float fy, float cx, float cy, float znear,
                                  float zfar, float* uv, float* conic, float* depth, int32_t* rect, int32_t* count, void* stream) {
    MUDG_REQUIRE(points && cov && opacity && mats && uv && conic && depth && rect && count, "mudg_gauss_project: null argument");
    MUDG_REQUIRE(aligned16(points), "mudg_gauss_project: unaligned points");
    MUDG_REQUIRE(aligned16(conic) && aligned16(rect) && (reinterpret_cast<uintptr_t>(uv) & 7u) == 0, "mudg_gauss_project: unaligned outputs");
    MUDG_REQUIRE(nmat > 0, "mudg_gauss_project: %d matrices per view", nmat);
    if (const int e = check_views("mudg_gauss_project", n, V, H, W)) return e;
    MUDG_REQUIRE(ids || nmat == 1, "mudg_gauss_project: %d matrices per view need per-point ids", nmat);
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_project: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    MUDG_REQUIRE(std::isfinite(znear) && std::isfinite(zfar) && znear > 0.0f && zfar > znear,
                 "mudg_gauss_project: need finite 0 < znear < zfar (positive depths order like their bits)");
    MUDG_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0f && fy > 0.0f && std::isfinite(cx) && std::isfinite(cy),
                 "mudg_gauss_project: intrinsics %g %g %g %g", (double)fx, (double)fy, (double)cx, (double)cy);
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
    MUDG_REQUIRE(grid_ok(total), "mudg_gauss_keys: %lld (view, Gaussian) pairs are more workgroups than a grid holds", (long long)total);
    hipLaunchKernelGGL(gauss_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth,
                       reinterpret_cast<const u32x4*>(rect), count, offsets, n, total, (W + TILE - 1) / TILE, (H + TILE - 1) / TILE, E,
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
    MUDG_REQUIRE(aligned16(conic) && (reinterpret_cast<uintptr_t>(uv) & 7u) == 0, "mudg_gauss_blend: unaligned projections");
    if (const int e = check_views("mudg_gauss_blend", n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_blend: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const int TX = (W + TILE - 1) / TILE, NT = TX * ((H + TILE - 1) / TILE);
    hipLaunchKernelGGL(gauss_blend_kernel, dim3((unsigned)((int64_t)V * NT)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t*>(points), reinterpret_cast<const f32x2*>(uv), reinterpret_cast<const f32x4*>(conic), depth,
                       values_sorted, ranges, n, E, TX, NT, H, W, rgb, depth_out, alpha, walked);
    return mudg_check_launch("mudg_gauss_blend");
}
