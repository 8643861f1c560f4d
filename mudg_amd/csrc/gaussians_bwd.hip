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
// Everything is fp32, each operation a single rounded one in the order DESIGN.md §24 writes it, so the gradients are bit-equal to the
// numpy definition in tests/gaussians_bwd_reference.py and a repeat run gives the same bits.  No MFMA operand is touched.
#include "gauss_shared.h"

namespace {

constexpr int SUMS = 10;                            // dcolour0..2, dzc, dopacity, dA, dB, dC, du, dv

// An entry in LDS is 48 bytes: (u, v, A, B), (C, opacity, zc, -) and (colour0, colour1, colour2, -).  A sorted value outside the cloud
// becomes an entry of opacity 0, which every pixel skips.
__device__ __forceinline__ void stage_entry(const f32x2* __restrict__ uv, const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                            const float* __restrict__ colour, const int32_t* __restrict__ values, int64_t view, int64_t n,
                                            int64_t e, int64_t end, f32x4& g0, f32x4& g1, f32x4& g2) {
    g0 = {0.0f, 0.0f, 0.0f, 0.0f};
    g1 = {0.0f, 0.0f, 0.0f, 0.0f};
    g2 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e < end) {
        const int64_t g = values[e];
        if (g >= 0 && g < n) {
            const int64_t o = view * n + g;
            const f32x2 p = uv[o];
            const f32x4 k = conic[o];
            g0.x = p.x; g0.y = p.y; g0.z = k.x; g0.w = k.y;
            g1.x = k.z; g1.y = k.w; g1.z = depth[o];
            g2.x = colour[3 * g]; g2.y = colour[3 * g + 1]; g2.z = colour[3 * g + 2];
        }
    }
}

__global__ __launch_bounds__(256) void gauss_blend_train_kernel(const float* __restrict__ colour, const f32x2* __restrict__ uv,
                                                                 const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                                 const int32_t* __restrict__ values, const int32_t* __restrict__ ranges,
                                                                 int64_t n, int64_t E, int TX, int NT, int H, int W, float* __restrict__ rgb,
                                                                 float* __restrict__ depth_out, float* __restrict__ alpha_out,
                                                                 float* __restrict__ state) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    __shared__ f32x4 tint[BATCH];
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
    for (int64_t base = start; base < end; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch has been read by every lane
        f32x4 g0, g1, g2;
        stage_entry(uv, conic, depth, colour, values, view, n, base + threadIdx.x, end, g0, g1, g2);
        geom[threadIdx.x] = g0;
        look[threadIdx.x] = g1;
        tint[threadIdx.x] = g2;
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
            const f32x4 c = tint[k];
            c0 = add(c0, mul(c.x, w));
            c1 = add(c1, mul(c.y, w));
            c2 = add(c2, mul(c.z, w));
            D = add(D, mul(b.z, w));
            T = Tn;
        }
    }
    if (inside) {
        const int64_t plane = (int64_t)H * W, pix = (int64_t)j * W + i;
        float* out = rgb + view * 3 * plane + pix;
        out[0] = dvd(c0, 255.0f);
        out[plane] = dvd(c1, 255.0f);
        out[2 * plane] = dvd(c2, 255.0f);
        depth_out[view * plane + pix] = D;
        alpha_out[view * plane + pix] = sub(1.0f, T);
        float* st = state + view * 5 * plane + pix;
        st[0] = c0;
        st[plane] = c1;
        st[2 * plane] = c2;
        st[3 * plane] = D;
        st[4 * plane] = T;
    }
}

// order[e]: the unsorted position of sorted entry e (the forward sort's permutation); a value outside [0, E) writes nothing.  Every entry
// of a batch that was staged gets its partial stored, +0.0 where no pixel blends it; the batches never staged keep the entry point's zeros.
__global__ __launch_bounds__(256) void gauss_blend_bwd_kernel(const float* __restrict__ colour, const f32x2* __restrict__ uv,
                                                               const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                               const int32_t* __restrict__ values, const int64_t* __restrict__ order,
                                                               const int32_t* __restrict__ ranges, int64_t n, int64_t E, int TX, int NT, int H,
                                                               int W, const float* __restrict__ state, const float* __restrict__ d_rgb,
                                                               const float* __restrict__ d_depth, const float* __restrict__ d_alpha,
                                                               float* __restrict__ partial) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    __shared__ f32x4 tint[BATCH];
    __shared__ float wsum[4 * BATCH * SUMS];                                // the four waves' sums of every entry of the batch
    const int64_t t = blockIdx.x;
    const int64_t view = t / NT;
    const int tile = (int)(t - view * NT);
    const int i = (tile % TX) * TILE + (threadIdx.x & (TILE - 1)), j = (tile / TX) * TILE + (threadIdx.x >> 4);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool inside = i < W && j < H;
    int64_t start = ranges[2 * t], end = ranges[2 * t + 1];
    if (start < 0 || end > E || start > end) start = end = 0;              // not a range of this call's entries
    const float px = add((float)i, 0.5f), py = add((float)j, 0.5f);
    float gC0 = 0.0f, gC1 = 0.0f, gC2 = 0.0f, gD = 0.0f, gAT = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sD = 0.0f;
    if (inside) {
        const int64_t plane = (int64_t)H * W, pix = (int64_t)j * W + i;
        const float* g = d_rgb + view * 3 * plane + pix;
        gC0 = dvd(g[0], 255.0f);
        gC1 = dvd(g[plane], 255.0f);
        gC2 = dvd(g[2 * plane], 255.0f);
        gD = d_depth[view * plane + pix];
        const float* st = state + view * 5 * plane + pix;
        s0 = st[0]; s1 = st[plane]; s2 = st[2 * plane]; sD = st[3 * plane];
        gAT = mul(d_alpha[view * plane + pix], st[4 * plane]);             // gA T_final
    }
    float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, D = 0.0f;
    int done = inside ? 0 : 1;
    for (int64_t base = start; base < end; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch and its sums have been read
        f32x4 g0, g1, g2;
        stage_entry(uv, conic, depth, colour, values, view, n, base + threadIdx.x, end, g0, g1, g2);
        geom[threadIdx.x] = g0;
        look[threadIdx.x] = g1;
        tint[threadIdx.x] = g2;
        __syncthreads();
        const int m = (int)(end - base < BATCH ? end - base : BATCH);
        for (int k = 0; k < m; ++k) {                                       // every lane walks every entry: the reduction needs them all
            float r[SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            bool blends = false;
            if (!done) {
                const f32x4 a = geom[k], b = look[k];
                const float dx = sub(a.x, px), dy = sub(a.y, py);
                const float q = add(mul(mul(a.z, dx), dx), mul(mul(b.x, dy), dy));
                const float p = sub(mul(-0.5f, q), mul(mul(a.w, dx), dy));
                if (!(p > 0.0f || p < MIN_POWER)) {
                    const float ge = gauss_exp(p);
                    const float raw = mul(b.y, ge);
                    const float al = fminf(MAX_ALPHA, raw);
                    if (!(al < MIN_ALPHA)) {
                        const float om = sub(1.0f, al);
                        const float Tn = mul(T, om);
                        if (Tn < MIN_T) {
                            done = 1;
                        } else {
                            blends = true;
                            const f32x4 c = tint[k];
                            const float w = mul(al, T);
                            c0 = add(c0, mul(c.x, w));
                            c1 = add(c1, mul(c.y, w));
                            c2 = add(c2, mul(c.z, w));
                            D = add(D, mul(b.z, w));
                            r[0] = mul(gC0, w);
                            r[1] = mul(gC1, w);
                            r[2] = mul(gC2, w);
                            r[3] = mul(gD, w);
                            if (!(raw > MAX_ALPHA)) {                       // the cap passes no gradient
                                const float own = add(add(add(mul(gC0, c.x), mul(gC1, c.y)), mul(gC2, c.z)), mul(gD, b.z));
                                const float behind = add(add(add(mul(gC0, sub(s0, c0)), mul(gC1, sub(s1, c1))), mul(gC2, sub(s2, c2))),
                                                         mul(gD, sub(sD, D)));
                                const float dal = add(sub(mul(T, own), dvd(behind, om)), dvd(gAT, om));
                                r[4] = mul(dal, ge);
                                const float dp = mul(mul(dal, b.y), ge);
                                r[5] = mul(dp, mul(-0.5f, mul(dx, dx)));
                                r[6] = mul(dp, -mul(dx, dy));
                                r[7] = mul(dp, mul(-0.5f, mul(dy, dy)));
                                r[8] = mul(dp, -add(mul(a.z, dx), mul(a.w, dy)));
                                r[9] = mul(dp, -add(mul(b.x, dy), mul(a.w, dx)));
                            }
                            T = Tn;
                        }
                    }
                }
            }
            float* out = wsum + ((size_t)wave * BATCH + k) * SUMS;
            if (__ballot(blends) != 0) {                                    // else: sixty-four times +0.0 is +0.0
#pragma unroll
                for (int c = 0; c < SUMS; ++c) {
#pragma unroll
                    for (int s = 1; s < 64; s <<= 1) r[c] = add(r[c], __shfl_xor(r[c], s));
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < SUMS; ++c) out[c] = r[c];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const int64_t at = order[base + threadIdx.x];
            if (at >= 0 && at < E) {
                float* out = partial + at * SUMS;
#pragma unroll
                for (int c = 0; c < SUMS; ++c) {
                    const int k = threadIdx.x * SUMS + c;
                    out[c] = add(add(add(wsum[k], wsum[BATCH * SUMS + k]), wsum[2 * BATCH * SUMS + k]), wsum[3 * BATCH * SUMS + k]);
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
    const u32x4 q = pts[idx];
    const float x = __uint_as_float(q.x), y = __uint_as_float(q.y), z = __uint_as_float(q.z);
    const float sxx = cov[6 * idx], sxy = cov[6 * idx + 1], sxz = cov[6 * idx + 2], syy = cov[6 * idx + 3], syz = cov[6 * idx + 4],
                szz = cov[6 * idx + 5];
    const float s[3][3] = {{sxx, sxy, sxz}, {sxy, syy, syz}, {sxz, syz, szz}};
    int id = 0;
    if (ids) { id = ids[idx]; id = id < 0 ? 0 : (id >= nmat ? nmat - 1 : id); }
    const float limx = mul(1.3f, dvd(mul(0.5f, (float)W), cam.fx)), limy = mul(1.3f, dvd(mul(0.5f, (float)H), cam.fy));
    float gx = 0.0f, gy = 0.0f, gz = 0.0f, gop = 0.0f, gc0 = 0.0f, gc1 = 0.0f, gc2 = 0.0f;
    float gs[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int view = 0; view < V; ++view) {
        const int64_t o = (int64_t)view * n + idx;
        const int cnt = count[o];
        if (cnt <= 0) continue;                                             // dropped in this view
        const int64_t off = offsets[o];
        if (off < 0 || off > E - cnt) continue;                             // not this call's entries
        const float* m = mats + ((int64_t)view * nmat + id) * 12;
        const float xc = add(add(add(mul(m[0], x), mul(m[1], y)), mul(m[2], z)), m[3]);
        const float yc = add(add(add(mul(m[4], x), mul(m[5], y)), mul(m[6], z)), m[7]);
        const float zc = add(add(add(mul(m[8], x), mul(m[9], y)), mul(m[10], z)), m[11]);
        if (!(zc > cam.znear && zc < cam.zfar)) continue;
        float acc[SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < cnt; ++k) {
            const float* p = partial + (off + k) * SUMS;
#pragma unroll
            for (int c = 0; c < SUMS; ++c) acc[c] = add(acc[c], p[c]);
        }
        gc0 = add(gc0, acc[0]);
        gc1 = add(gc1, acc[1]);
        gc2 = add(gc2, acc[2]);
        gop = add(gop, acc[4]);
        // the forward's values (§23 steps 2 - 9)
        const float qx = dvd(xc, zc), qy = dvd(yc, zc);
        const float kx = fminf(limx, fmaxf(-limx, qx)), ky = fminf(limy, fmaxf(-limy, qy));
        const float tx = mul(kx, zc), ty = mul(ky, zc);
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
        const float A = dvd(c, det), B = -dvd(b, det), C = dvd(a, det);
        // conic -> (a, b, c): with K the conic and G = [[gA, gB / 2], [gB / 2, gC]], d(a, b, c) = -(K G K) read as (00, 2 x 01, 11)
        const float gA = acc[5], hB = mul(0.5f, acc[6]), gC = acc[7];
        const float x00 = add(mul(gA, A), mul(hB, B)), x01 = add(mul(gA, B), mul(hB, C));
        const float x10 = add(mul(hB, A), mul(gC, B)), x11 = add(mul(hB, B), mul(gC, C));
        const float da = -add(mul(A, x00), mul(B, x10));
        const float db = mul(-2.0f, add(mul(A, x01), mul(B, x11)));
        const float dc = -add(mul(B, x01), mul(C, x11));
        const float da2 = mul(2.0f, da), dc2 = mul(2.0f, dc);
        // (a, b, c) -> the covariance (off-diagonal entries: both halves) and T = J R
        int e = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = r; k < 3; ++k, ++e) {
                float g;
                if (r == k)
                    g = add(add(mul(da, mul(t0[r], t0[r])), mul(db, mul(t0[r], t1[r]))), mul(dc, mul(t1[r], t1[r])));
                else
                    g = add(add(mul(da2, mul(t0[r], t0[k])), mul(db, add(mul(t0[r], t1[k]), mul(t0[k], t1[r])))), mul(dc2, mul(t1[r], t1[k])));
                gs[e] = add(gs[e], g);
            }
        }
        float dt0[3], dt1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dt0[k] = add(mul(da2, v0[k]), mul(db, v1[k]));
            dt1[k] = add(mul(dc2, v1[k]), mul(db, v0[k]));
        }
        // T -> j00, j02, j11, j12
        const float dj00 = add(add(mul(dt0[0], m[0]), mul(dt0[1], m[1])), mul(dt0[2], m[2]));
        const float dj02 = add(add(mul(dt0[0], m[8]), mul(dt0[1], m[9])), mul(dt0[2], m[10]));
        const float dj11 = add(add(mul(dt1[0], m[4]), mul(dt1[1], m[5])), mul(dt1[2], m[6]));
        const float dj12 = add(add(mul(dt1[0], m[8]), mul(dt1[1], m[9])), mul(dt1[2], m[10]));
        // j -> xc, yc, zc
        const float dtx = -dvd(mul(dj02, cam.fx), zz), dty = -dvd(mul(dj12, cam.fy), zz);
        const float dzz = -add(dvd(mul(dj02, j02), zz), dvd(mul(dj12, j12), zz));
        float dzc = acc[3];                                                 // the depth term
        dzc = sub(dzc, dvd(mul(dj00, j00), zc));
        dzc = sub(dzc, dvd(mul(dj11, j11), zc));
        dzc = add(dzc, mul(mul(2.0f, zc), dzz));
        dzc = add(dzc, mul(dtx, kx));
        dzc = add(dzc, mul(dty, ky));
        float dqx = mul(acc[8], cam.fx), dqy = mul(acc[9], cam.fy);
        if (kx == qx) dqx = add(dqx, mul(dtx, zc));                         // a clamped tx passes nothing through xc / zc
        if (ky == qy) dqy = add(dqy, mul(dty, zc));
        const float dxc = dvd(dqx, zc), dyc = dvd(dqy, zc);
        dzc = sub(dzc, dvd(mul(dqx, qx), zc));
        dzc = sub(dzc, dvd(mul(dqy, qy), zc));
        gx = add(gx, add(add(mul(dxc, m[0]), mul(dyc, m[4])), mul(dzc, m[8])));
        gy = add(gy, add(add(mul(dxc, m[1]), mul(dyc, m[5])), mul(dzc, m[9])));
        gz = add(gz, add(add(mul(dxc, m[2]), mul(dyc, m[6])), mul(dzc, m[10])));
    }
    d_xyz[3 * idx] = gx; d_xyz[3 * idx + 1] = gy; d_xyz[3 * idx + 2] = gz;
#pragma unroll
    for (int k = 0; k < 6; ++k) d_cov[6 * idx + k] = gs[k];
    d_opacity[idx] = gop;
    d_colour[3 * idx] = gc0; d_colour[3 * idx + 1] = gc1; d_colour[3 * idx + 2] = gc2;
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int mudg_gauss_blend_train(const float* colour, const float* uv, const float* conic, const float* depth,
                                      const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb,
                                      float* depth_out, float* alpha, float* state, void* stream) {
    MUDG_REQUIRE(colour && uv && conic && depth && values_sorted && ranges && rgb && depth_out && alpha && state,
                 "mudg_gauss_blend_train: null argument");
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv), "mudg_gauss_blend_train: unaligned projections");
    if (const int e = check_views("mudg_gauss_blend_train", n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_blend_train: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const int TX = (W + TILE - 1) / TILE, NT = TX * ((H + TILE - 1) / TILE);
    hipLaunchKernelGGL(gauss_blend_train_kernel, dim3((unsigned)((int64_t)V * NT)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), colour,
                       reinterpret_cast<const f32x2*>(uv), reinterpret_cast<const f32x4*>(conic), depth, values_sorted, ranges, n, E, TX, NT, H, W,
                       rgb, depth_out, alpha, state);
    return mudg_check_launch("mudg_gauss_blend_train");
}

extern "C" int mudg_gauss_blend_bwd(const float* colour, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                                    const int64_t* order, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, const float* state,
                                    const float* d_rgb, const float* d_depth, const float* d_alpha, float* partial, void* stream) {
    MUDG_REQUIRE(colour && uv && conic && depth && values_sorted && order && ranges && state && d_rgb && d_depth && d_alpha && partial,
                 "mudg_gauss_blend_bwd: null argument");
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv) && aligned8(order), "mudg_gauss_blend_bwd: unaligned projections or order");
    if (const int e = check_views("mudg_gauss_blend_bwd", n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_blend_bwd: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const int TX = (W + TILE - 1) / TILE, NT = TX * ((H + TILE - 1) / TILE);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(partial, 0, (size_t)E * SUMS * sizeof(float), s) != hipSuccess) return mudg_check_launch("mudg_gauss_blend_bwd");
    hipLaunchKernelGGL(gauss_blend_bwd_kernel, dim3((unsigned)((int64_t)V * NT)), dim3(256), 0, s, colour, reinterpret_cast<const f32x2*>(uv),
                       reinterpret_cast<const f32x4*>(conic), depth, values_sorted, order, ranges, n, E, TX, NT, H, W, state, d_rgb, d_depth,
                       d_alpha, partial);
    return mudg_check_launch("mudg_gauss_blend_bwd");
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
    MUDG_REQUIRE(std::isfinite(znear) && std::isfinite(zfar) && znear > 0.0f && zfar > znear,
                 "mudg_gauss_project_bwd: need finite 0 < znear < zfar");
    MUDG_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0f && fy > 0.0f && std::isfinite(cx) && std::isfinite(cy),
                 "mudg_gauss_project_bwd: intrinsics %g %g %g %g", (double)fx, (double)fy, (double)cx, (double)cy);
    const GaussCam cam = {fx, fy, cx, cy, znear, zfar};
    hipLaunchKernelGGL(gauss_project_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(points), cov, ids, mats, n, V, nmat, H, W, cam, count, offsets, partial, E, d_xyz, d_cov,
                       d_opacity, d_colour);
    return mudg_check_launch("mudg_gauss_project_bwd");
}
