// gaussians_bwd.hip — the training half of the Gaussian splat renderer: a forward blend that keeps what a backward needs,
// and the backward of the blend and of the projection.
//   gauss_blend_train  gauss_blend (§23) with the colour read from an fp32 (n, 3) tensor in byte units; besides the images it stores the
//                      raw accumulators (C0, C1, C2, D, T) of every pixel
//   gauss_blend_bwd    a workgroup owns a tile, a lane a pixel, as in the forward.  It walks the tile's entries front to back, recomputes
//                      what the forward computed with the forward's operations, and reduces the ten per-entry sums over the tile's 256
//                      pixels in one fixed order: an xor butterfly inside each wave, the four waves through LDS as ((w0 + w1) + w2) + w3.
//                      The result is stored at the entry's unsorted position; no atomics on global memory
//   gauss_project_bwd  a lane owns a Gaussian: per view it sums the Gaussian's partials in ascending order and applies the chain rule
//                      through the projection of §23; the views are added in view order
// The two blends also serve DESIGN.md §27's entry points (`_views`): there the colour tensor is (V, n, 3) and per_view, the floats from
// one view's colours to the next, is 3 n; for one colour per Gaussian it is 0.  The inference blend of §27 is gauss_blend_train without
// a state pointer.
// Everything is fp32, each operation a single rounded one in the order DESIGN.md §24 writes it, so the gradients are bit-equal to the
// numpy definition in tests/gaussians_bwd_reference.py and a repeat run gives the same bits.  No MFMA operand is touched.
#include "gauss_shared.h"

namespace {

// An entry in LDS is 48 bytes: stage_batch's two words and (colour0, colour1, colour2, -).
__global__ __launch_bounds__(256) void gauss_blend_train_kernel(const float* __restrict__ colour, int64_t per_view, const f32x2* __restrict__ uv,
                                                                 const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                                 const int32_t* __restrict__ values, const int32_t* __restrict__ ranges,
                                                                 int64_t n, int64_t E, int TX, int NT, int H, int W, float* __restrict__ rgb,
                                                                 float* __restrict__ depth_out, float* __restrict__ alpha_out,
                                                                 float* __restrict__ state) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    __shared__ f32x4 tint[BATCH];
    const GaussTile tile = gauss_tile(blockIdx.x, ranges, E, TX, NT, H, W);
    GaussPixel acc;
    blend_forward(uv, conic, depth, values, n, tile, FloatColour{colour + tile.view * per_view, tint}, geom, look, acc);
    if (tile.inside) {
        store_images(tile, H, W, acc, rgb, depth_out, alpha_out);
        if (state) store_state(tile, H, W, acc, state);                    // NULL: inference, the images only
    }
}

// order[e]: the unsorted position of sorted entry e (the forward sort's permutation); a value outside [0, E) writes nothing.  Every entry
// of a batch that was staged gets its partial stored, +0.0 where no pixel blends it; the batches never staged keep the entry point's zeros.
__global__ __launch_bounds__(256) void gauss_blend_bwd_kernel(const float* __restrict__ colour, int64_t per_view, const f32x2* __restrict__ uv,
                                                               const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                               const int32_t* __restrict__ values, const int64_t* __restrict__ order,
                                                               const int32_t* __restrict__ ranges, int64_t n, int64_t E, int TX, int NT, int H,
                                                               int W, const float* __restrict__ state, const float* __restrict__ d_rgb,
                                                               const float* __restrict__ d_depth, const float* __restrict__ d_alpha,
                                                               float* __restrict__ partial) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    __shared__ f32x4 tint[BATCH];
    __shared__ float wsum[4 * BATCH * GAUSS_SUMS];                          // the four waves' sums of every entry of the batch
    const GaussTile tile = gauss_tile(blockIdx.x, ranges, E, TX, NT, H, W);
    const FloatColour tints = {colour + tile.view * per_view, tint};
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const GaussUpstream up = load_upstream(tile, H, W, state, d_rgb, d_depth, d_alpha);
    GaussPixel acc;
    int done = tile.inside ? 0 : 1;
    for (int64_t base = tile.start; base < tile.end; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch and its sums have been read
        stage_batch(uv, conic, depth, values, n, tile, base, tints, geom, look);
        const int m = (int)(tile.end - base < BATCH ? tile.end - base : BATCH);
        for (int k = 0; k < m; ++k) {                                       // every lane walks every entry: the reduction needs them all
            float r[GAUSS_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            bool blends = false;
            if (!done) {
                const f32x4 a = geom[k], b = look[k];
                done = blend_step(a, b, tile.px, tile.py, acc.T, [&](const GaussBlend& s) {
                    blends = true;
                    const f32x4 c = tints.at(k, b);
                    const float T = acc.T, zc = b.w;
                    accumulate(acc, c, zc, s);
                    blend_bwd_direct(up, s, r);
                    if (s.raw > MAX_ALPHA) return;                          // the cap passes no gradient
                    blend_bwd_alpha(up, a, b, s, T, blend_bwd_own(up, c, zc), blend_bwd_behind(up, acc), r);
                });
            }
            float* out = wsum + ((size_t)wave * BATCH + k) * GAUSS_SUMS;
            if (__ballot(blends) != 0) {                                    // else: sixty-four times +0.0 is +0.0
#pragma unroll
                for (int c = 0; c < GAUSS_SUMS; ++c) r[c] = butterfly_sum(r[c]);
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < GAUSS_SUMS; ++c) out[c] = r[c];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const int64_t at = order[base + threadIdx.x];
            if (at >= 0 && at < E) {
                float* out = partial + at * GAUSS_SUMS;
#pragma unroll
                for (int c = 0; c < GAUSS_SUMS; ++c) {
                    const float* w = wsum + threadIdx.x * GAUSS_SUMS + c;
                    out[c] = four_waves(w[0], w[BATCH * GAUSS_SUMS], w[2 * BATCH * GAUSS_SUMS], w[3 * BATCH * GAUSS_SUMS]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void gauss_project_bwd_kernel(const u32x4* __restrict__ pts, const float* __restrict__ cov,
                                                                 const int32_t* __restrict__ ids, const float* __restrict__ mats, int64_t n,
                                                                 int V, int nmat, int H, int W, GaussCam cam, const int32_t* __restrict__ count,
                                                                 const int64_t* __restrict__ offsets, const float* __restrict__ partial,
                                                                 int64_t E, float* __restrict__ d_xyz, float* __restrict__ d_cov,
                                                                 float* __restrict__ d_opacity, float* __restrict__ d_colour) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const GaussPoint p = load_gaussian(pts, cov, ids, nmat, idx);
    const float limx = gauss_limit(W, cam.fx), limy = gauss_limit(H, cam.fy);
    float gx = 0.0f, gy = 0.0f, gz = 0.0f, gop = 0.0f, gc0 = 0.0f, gc1 = 0.0f, gc2 = 0.0f;
    float gs[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int view = 0;
    const auto chain = [&](const float (&acc)[GAUSS_SUMS]) {               // the sums of this view's partials through the chain rule
        const float* m = mats + ((int64_t)view * nmat + p.id) * 12;
        GaussView w;                                                        // the forward's values (§23 steps 2 - 9)
        if (!gauss_view(m, p, cam, limx, limy, w)) return;
        gc0 = add(gc0, acc[SUM_COLOUR]);
        gc1 = add(gc1, acc[SUM_COLOUR + 1]);
        gc2 = add(gc2, acc[SUM_COLOUR + 2]);
        gop = add(gop, acc[SUM_OPACITY]);
        GaussViewBwd b;                                                     // the chain rule, written once (gauss_shared.h)
        gauss_view_bwd(m, w, cam, acc, b);
#pragma unroll
        for (int e = 0; e < 6; ++e) gs[e] = add(gs[e], b.dcov[e]);
        const float dxc = b.dxc, dyc = b.dyc, dzc = b.dzc;
        gx = add(gx, add(add(mul(dxc, m[0]), mul(dyc, m[4])), mul(dzc, m[8])));
        gy = add(gy, add(add(mul(dxc, m[1]), mul(dyc, m[5])), mul(dzc, m[9])));
        gz = add(gz, add(add(mul(dxc, m[2]), mul(dyc, m[6])), mul(dzc, m[10])));
    };
    for (; view < V; ++view) with_partials<0, GAUSS_SUMS>(partial, count, offsets, (int64_t)view * n + idx, E, chain);
    d_xyz[3 * idx] = gx; d_xyz[3 * idx + 1] = gy; d_xyz[3 * idx + 2] = gz;
#pragma unroll
    for (int k = 0; k < 6; ++k) d_cov[6 * idx + k] = gs[k];
    d_opacity[idx] = gop;
    d_colour[3 * idx] = gc0; d_colour[3 * idx + 1] = gc1; d_colour[3 * idx + 2] = gc2;
}

}  // namespace

// The two float-colour blends behind their entry points: `name` speaks in the refusals, per_view is 0 for one colour per Gaussian and 3 n
// for one per (view, Gaussian) (§27), state may be NULL only for the inference blend.
static int blend_train(const char* name, const float* colour, int64_t per_view, const float* uv, const float* conic, const float* depth,
                       const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb,
                       float* depth_out, float* alpha, float* state, bool with_state, void* stream) {
    MUDG_REQUIRE(colour && uv && conic && depth && values_sorted && ranges && rgb && depth_out && alpha && (state || !with_state),
                 "%s: null argument", name);
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv), "%s: unaligned projections", name);
    if (const int e = check_views(name, n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "%s: %lld entries (1 .. 2^31 - 1)", name, (long long)E);
    const GaussGrid grid(H, W);
    hipLaunchKernelGGL(gauss_blend_train_kernel, dim3((unsigned)((int64_t)V * grid.NT)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), colour,
                       per_view, reinterpret_cast<const f32x2*>(uv), reinterpret_cast<const f32x4*>(conic), depth, values_sorted, ranges, n, E,
                       grid.TX, grid.NT, H, W, rgb, depth_out, alpha, with_state ? state : nullptr);
    return mudg_check_launch(name);
}

static int blend_bwd(const char* name, const float* colour, int64_t per_view, const float* uv, const float* conic, const float* depth,
                     const int32_t* values_sorted, const int64_t* order, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W,
                     const float* state, const float* d_rgb, const float* d_depth, const float* d_alpha, float* partial, void* stream) {
    MUDG_REQUIRE(colour && uv && conic && depth && values_sorted && order && ranges && state && d_rgb && d_depth && d_alpha && partial,
                 "%s: null argument", name);
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv) && aligned8(order), "%s: unaligned projections or order", name);
    if (const int e = check_views(name, n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "%s: %lld entries (1 .. 2^31 - 1)", name, (long long)E);
    const GaussGrid grid(H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(partial, 0, (size_t)E * GAUSS_SUMS * sizeof(float), s) != hipSuccess) return mudg_check_launch(name);
    hipLaunchKernelGGL(gauss_blend_bwd_kernel, dim3((unsigned)((int64_t)V * grid.NT)), dim3(256), 0, s, colour, per_view,
                       reinterpret_cast<const f32x2*>(uv), reinterpret_cast<const f32x4*>(conic), depth, values_sorted, order, ranges, n, E, grid.TX,
                       grid.NT, H, W, state, d_rgb, d_depth, d_alpha, partial);
    return mudg_check_launch(name);
}

extern "C" int mudg_gauss_blend_train(const float* colour, const float* uv, const float* conic, const float* depth,
                                      const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb,
                                      float* depth_out, float* alpha, float* state, void* stream) {
    return blend_train("mudg_gauss_blend_train", colour, 0, uv, conic, depth, values_sorted, ranges, n, E, V, H, W, rgb, depth_out, alpha, state,
                       true, stream);
}

extern "C" int mudg_gauss_blend_bwd(const float* colour, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                                    const int64_t* order, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, const float* state,
                                    const float* d_rgb, const float* d_depth, const float* d_alpha, float* partial, void* stream) {
    return blend_bwd("mudg_gauss_blend_bwd", colour, 0, uv, conic, depth, values_sorted, order, ranges, n, E, V, H, W, state, d_rgb, d_depth,
                     d_alpha, partial, stream);
}

// §27: colours (V, n, 3), one colour per (view, Gaussian); everything else as the three blends above
extern "C" int mudg_gauss_blend_views(const float* colours, const float* uv, const float* conic, const float* depth,
                                      const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb,
                                      float* depth_out, float* alpha, void* stream) {
    return blend_train("mudg_gauss_blend_views", colours, 3 * n, uv, conic, depth, values_sorted, ranges, n, E, V, H, W, rgb, depth_out, alpha,
                       nullptr, false, stream);
}

extern "C" int mudg_gauss_blend_train_views(const float* colours, const float* uv, const float* conic, const float* depth,
                                            const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W,
                                            float* rgb, float* depth_out, float* alpha, float* state, void* stream) {
    return blend_train("mudg_gauss_blend_train_views", colours, 3 * n, uv, conic, depth, values_sorted, ranges, n, E, V, H, W, rgb, depth_out,
                       alpha, state, true, stream);
}

extern "C" int mudg_gauss_blend_bwd_views(const float* colours, const float* uv, const float* conic, const float* depth,
                                          const int32_t* values_sorted, const int64_t* order, const int32_t* ranges, int64_t n, int64_t E, int V,
                                          int H, int W, const float* state, const float* d_rgb, const float* d_depth, const float* d_alpha,
                                          float* partial, void* stream) {
    return blend_bwd("mudg_gauss_blend_bwd_views", colours, 3 * n, uv, conic, depth, values_sorted, order, ranges, n, E, V, H, W, state, d_rgb,
                     d_depth, d_alpha, partial, stream);
}

extern "C" int mudg_gauss_project_bwd(const void* points, const float* cov, const int32_t* ids, int64_t n, const float* mats, int V, int nmat,
                                      int H, int W, float fx, float fy, float cx, float cy, float znear, float zfar, const int32_t* count,
                                      const int64_t* offsets, const float* partial, int64_t E, float* d_xyz, float* d_cov, float* d_opacity,
                                      float* d_colour, void* stream) {
    MUDG_REQUIRE(points && cov && mats && count && offsets && partial && d_xyz && d_cov && d_opacity && d_colour,
                 "mudg_gauss_project_bwd: null argument");
    MUDG_REQUIRE(aligned16(points), "mudg_gauss_project_bwd: unaligned points");
    MUDG_REQUIRE(aligned8(offsets), "mudg_gauss_project_bwd: unaligned offsets");
    MUDG_REQUIRE(nmat > 0, "mudg_gauss_project_bwd: %d matrices per view", nmat);
    if (const int e = check_views("mudg_gauss_project_bwd", n, V, H, W)) return e;
    MUDG_REQUIRE(ids || nmat == 1, "mudg_gauss_project_bwd: %d matrices per view need per-point ids", nmat);
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_project_bwd: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_project_bwd: %lld entries (1 .. 2^31 - 1)", (long long)E);
    if (const int e = check_camera("mudg_gauss_project_bwd", fx, fy, cx, cy, znear, zfar)) return e;
    const GaussCam cam = {fx, fy, cx, cy, znear, zfar};
    hipLaunchKernelGGL(gauss_project_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(points), cov, ids, mats, n, V, nmat, H, W, cam, count, offsets, partial, E, d_xyz, d_cov,
                       d_opacity, d_colour);
    return mudg_check_launch("mudg_gauss_project_bwd");
}
