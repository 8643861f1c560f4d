// gauss_shared.h — every step that more than one kernel of the Gaussian splat renderer computes (gaussians.hip, DESIGN.md §23;
// gaussians_bwd.hip, §24; gaussians_density.hip, §25; gaussians_loss.hip, §26; gaussians_sh.hip, §27; gaussians_feat.hip, §29), written once: the constants of the rule, the single
// rounded operations, the polynomial exponential, a Gaussian's load and its projection into a view, a tile's prologue, the staging of an
// entry, the blend step and the forward blend loop, a pixel's state and the blend's backward at a pixel, the walk over a Gaussian's partials, the fixed-order tile reduction, and the checks
// the entry points share, the chain rule of one (view, Gaussian) (§24) and the fixed-order reduction over all Gaussians of a (view, matrix)
// (§28).  One copy, so that the backward recomputes the forward's values bit for bit.
#pragma once
#include "splat_shared.h"

#include <cmath>

constexpr int TILE = 16;                            // pixels a side; a workgroup of 256 lanes is one tile
constexpr int BATCH = 256;                          // entries staged through LDS at a time
constexpr float MAX_RADIUS = 4096.0f;               // a footprint beyond this is dropped (keeps the integer conversion safe)
constexpr float MIN_ALPHA = 1.0f / 255.0f;
constexpr float MAX_ALPHA = 0.99f;
constexpr float MIN_POWER = -5.55f;                 // e^-5.55 < 1 / 255
constexpr float MIN_T = 1e-4f;
constexpr float BLUR = 0.3f;                        // added to the diagonal of the 2-D covariance
constexpr float LOG2E = 1.44269504f;
constexpr int GAUSS_SUMS = 10;                      // a partial's row: the sums over a tile's pixels for one entry, in these columns
constexpr int SUM_COLOUR = 0, SUM_ZC = 3, SUM_OPACITY = 4, SUM_A = 5, SUM_B = 6, SUM_C = 7, SUM_U = 8, SUM_V = 9;

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float dvd(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }     // not a number -> lo

// 2^(p log2 e) for -5.6 <= p <= 0: the integer part by ldexp (exact), the fraction by a degree-5 polynomial in Horner form.
__device__ __forceinline__ float gauss_exp(float p) {
    const float t = mul(p, LOG2E);
    const float n = floorf(t);
    const float f = sub(t, n);                      // exact
    float r = 0x1.f06faep-10f;
    r = add(mul(r, f), 0x1.25429cp-7f);
    r = add(mul(r, f), 0x1.c99b9ep-5f);
    r = add(mul(r, f), 0x1.ebcf7ap-3f);
    r = add(mul(r, f), 0x1.62e526p-1f);
    r = add(mul(r, f), 1.0f);
    return ldexpf(r, (int)n);
}

struct GaussCam { float fx, fy, cx, cy, znear, zfar; };

// ------------------------------------------------------------------------------------------------ a Gaussian and its projection (§23)
// The packed point (one 16-byte load), the symmetric covariance and the matrix id, clamped to the table.
struct GaussPoint {
    float x, y, z, s[3][3];
    int id;
};

__device__ __forceinline__ GaussPoint load_gaussian(const u32x4* __restrict__ pts, const float* __restrict__ cov,
                                                    const int32_t* __restrict__ ids, int nmat, int64_t idx) {
    const u32x4 q = pts[idx];
    const float sxx = cov[6 * idx], sxy = cov[6 * idx + 1], sxz = cov[6 * idx + 2], syy = cov[6 * idx + 3], syz = cov[6 * idx + 4],
                szz = cov[6 * idx + 5];
    GaussPoint g = {__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), {{sxx, sxy, sxz}, {sxy, syy, syz}, {sxz, syz, szz}}, 0};
    if (ids) { g.id = ids[idx]; g.id = g.id < 0 ? 0 : (g.id >= nmat ? nmat - 1 : g.id); }
    return g;
}

// the largest |x / z| (|y / z|) the Jacobian is evaluated at: 1.3 times the half image over the focal length
__device__ __forceinline__ float gauss_limit(int extent, float focal) { return mul(1.3f, dvd(mul(0.5f, (float)extent), focal)); }

// §23 steps 2 - 9 of one Gaussian through the 3 x 4 matrix m: false (and only xc, yc, zc set) when zc leaves the depth range.
struct GaussView {
    float xc, yc, zc, qx, qy, kx, ky, u, v, zz, j00, j02, j11, j12, t0[3], t1[3], v0[3], v1[3], a, b, c, det;
};

__device__ __forceinline__ bool gauss_view(const float* __restrict__ m, const GaussPoint& g, const GaussCam& cam, float limx, float limy,
                                           GaussView& w) {
    w.xc = add(add(add(mul(m[0], g.x), mul(m[1], g.y)), mul(m[2], g.z)), m[3]);
    w.yc = add(add(add(mul(m[4], g.x), mul(m[5], g.y)), mul(m[6], g.z)), m[7]);
    w.zc = add(add(add(mul(m[8], g.x), mul(m[9], g.y)), mul(m[10], g.z)), m[11]);
    if (!(w.zc > cam.znear && w.zc < cam.zfar)) return false;
    w.qx = dvd(w.xc, w.zc); w.qy = dvd(w.yc, w.zc);
    w.u = add(mul(cam.fx, w.qx), cam.cx); w.v = add(mul(cam.fy, w.qy), cam.cy);
    w.kx = fminf(limx, fmaxf(-limx, w.qx)); w.ky = fminf(limy, fmaxf(-limy, w.qy));
    const float tx = mul(w.kx, w.zc), ty = mul(w.ky, w.zc);
    w.zz = mul(w.zc, w.zc);
    w.j00 = dvd(cam.fx, w.zc); w.j02 = -dvd(mul(cam.fx, tx), w.zz);
    w.j11 = dvd(cam.fy, w.zc); w.j12 = -dvd(mul(cam.fy, ty), w.zz);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w.t0[k] = add(mul(w.j00, m[k]), mul(w.j02, m[8 + k]));
        w.t1[k] = add(mul(w.j11, m[4 + k]), mul(w.j12, m[8 + k]));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w.v0[k] = add(add(mul(w.t0[0], g.s[0][k]), mul(w.t0[1], g.s[1][k])), mul(w.t0[2], g.s[2][k]));
        w.v1[k] = add(add(mul(w.t1[0], g.s[0][k]), mul(w.t1[1], g.s[1][k])), mul(w.t1[2], g.s[2][k]));
    }
    w.a = add(add(add(mul(w.v0[0], w.t0[0]), mul(w.v0[1], w.t0[1])), mul(w.v0[2], w.t0[2])), BLUR);
    w.b = add(add(mul(w.v0[0], w.t1[0]), mul(w.v0[1], w.t1[1])), mul(w.v0[2], w.t1[2]));
    w.c = add(add(add(mul(w.v1[0], w.t1[0]), mul(w.v1[1], w.t1[1])), mul(w.v1[2], w.t1[2])), BLUR);
    w.det = sub(mul(w.a, w.c), mul(w.b, w.b));
    return true;
}

// ------------------------------------------------------------------------------------------------ a tile and its entries
// Workgroup t of a grid of (group, tile) pairs, NT tiles a group in rows of TX: the group (a view; for the loss a view's channel) and
// the tile's column and row.
struct TileId {
    int64_t group;
    int ti, tj;
};

__device__ __forceinline__ TileId tile_id(int64_t t, int TX, int NT) {
    const int64_t group = t / NT;
    const int tile = (int)(t - group * NT);
    return {group, tile % TX, tile / TX};
}

// The blend kernels' prologue: the lane's pixel, whether the image has it, the pixel's centre, and the tile's [start, end) of sorted
// entries, empty where ranges does not hold a range of this call's E entries.
struct GaussTile {
    int64_t view, start, end;
    int i, j;
    bool inside;
    float px, py;
};

__device__ __forceinline__ GaussTile gauss_tile(int64_t t, const int32_t* __restrict__ ranges, int64_t E, int TX, int NT, int H, int W) {
    const TileId id = tile_id(t, TX, NT);
    GaussTile g;
    g.view = id.group;
    g.i = id.ti * TILE + (threadIdx.x & (TILE - 1));
    g.j = id.tj * TILE + (threadIdx.x >> 4);
    g.inside = g.i < W && g.j < H;
    g.start = ranges[2 * t];
    g.end = ranges[2 * t + 1];
    if (g.start < 0 || g.end > E || g.start > g.end) g.start = g.end = 0;
    g.px = add((float)g.i, 0.5f);
    g.py = add((float)g.j, 0.5f);
    return g;
}

// The colour of an entry, for the two forward blends and the backward.  ByteColour: the packed point's colour word travels in the free
// slot of the entry's second word and is unpacked per pixel.  FloatColour: an fp32 (n, 3) tensor in byte units, staged in a third LDS
// array.
struct ByteColour {
    const uint32_t* __restrict__ pts;
    __device__ __forceinline__ void load(int64_t g, f32x4& g1, f32x4&) const { g1.z = __uint_as_float(pts[4 * g + 3] & 0x00ffffffu); }
    __device__ __forceinline__ void store(const f32x4&) const {}
    __device__ __forceinline__ f32x4 at(int, const f32x4& g1) const {
        const uint32_t word = __float_as_uint(g1.z);
        return {(float)(word & 0xffu), (float)((word >> 8) & 0xffu), (float)((word >> 16) & 0xffu), 0.0f};
    }
};

struct FloatColour {
    const float* __restrict__ colour;
    f32x4* tint;                                    // LDS, BATCH entries
    __device__ __forceinline__ void load(int64_t g, f32x4&, f32x4& g2) const {
        g2.x = colour[3 * g]; g2.y = colour[3 * g + 1]; g2.z = colour[3 * g + 2];
    }
    __device__ __forceinline__ void store(const f32x4& g2) const { tint[threadIdx.x] = g2; }
    __device__ __forceinline__ f32x4 at(int k, const f32x4&) const { return tint[k]; }
};

// Lane l stages sorted entry base + l of the tile: geom[l] = (u, v, A, B), look[l] = (C, opacity, -, zc) with the free slot the
// colour's, and the colour's own array.  Past the tile's end and for a sorted value outside the cloud the entry is zeros (opacity 0:
// every pixel skips it).  Ends with the barrier after which every lane may read the batch.
template <class Colour>
__device__ __forceinline__ void stage_batch(const f32x2* __restrict__ uv, const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                            const int32_t* __restrict__ values, int64_t n, const GaussTile& tile, int64_t base,
                                            const Colour& colour, f32x4* geom, f32x4* look) {
    const int64_t e = base + threadIdx.x;
    f32x4 g0 = {0.0f, 0.0f, 0.0f, 0.0f}, g1 = {0.0f, 0.0f, 0.0f, 0.0f}, g2 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e < tile.end) {
        const int64_t g = values[e];
        if (g >= 0 && g < n) {
            const int64_t o = tile.view * n + g;
            const f32x2 p = uv[o];
            const f32x4 k = conic[o];
            g0.x = p.x; g0.y = p.y; g0.z = k.x; g0.w = k.y;
            g1.x = k.z; g1.y = k.w; g1.w = depth[o];
            colour.load(g, g1, g2);
        }
    }
    geom[threadIdx.x] = g0;
    look[threadIdx.x] = g1;
    colour.store(g2);
    __syncthreads();
}

// One staged entry (a, b) = (geom[k], look[k]) at the pixel whose centre is (px, py) and whose transmittance is T (§23 step 12).  The
// pixel skips the entry (false), blends it (blend(s) runs; false), or is opaque before it and ends (true).  s holds what the blend and
// its backward use.
struct GaussBlend {
    float dx, dy, ge, raw, al, om, Tn, w;           // ge = E(p), raw = opacity ge, al = min(0.99, raw), om = 1 - al, Tn = T om, w = al T
};

template <class Blend>
__device__ __forceinline__ bool blend_step(const f32x4& a, const f32x4& b, float px, float py, float T, Blend&& blend) {
    GaussBlend s;
    s.dx = sub(a.x, px); s.dy = sub(a.y, py);
    const float q = add(mul(mul(a.z, s.dx), s.dx), mul(mul(b.x, s.dy), s.dy));
    const float p = sub(mul(-0.5f, q), mul(mul(a.w, s.dx), s.dy));
    if (p > 0.0f || p < MIN_POWER) return false;
    s.ge = gauss_exp(p);
    s.raw = mul(b.y, s.ge);
    s.al = fminf(MAX_ALPHA, s.raw);
    if (s.al < MIN_ALPHA) return false;
    s.om = sub(1.0f, s.al);
    s.Tn = mul(T, s.om);
    if (s.Tn < MIN_T) return true;
    s.w = mul(s.al, T);
    blend(s);
    return false;
}

// A pixel's raw accumulators, and one blended entry added to them.
struct GaussPixel {
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, D = 0.0f, T = 1.0f;
};

__device__ __forceinline__ void accumulate(GaussPixel& acc, const f32x4& c, float zc, const GaussBlend& s) {
    acc.c0 = add(acc.c0, mul(c.x, s.w));
    acc.c1 = add(acc.c1, mul(c.y, s.w));
    acc.c2 = add(acc.c2, mul(c.z, s.w));
    acc.D = add(acc.D, mul(zc, s.w));
    acc.T = s.Tn;
}

// The forward blend of a tile: its entries through LDS in batches of BATCH, front to back, until every pixel of the tile is opaque.
// Returns the entries the workgroup staged before it left.
template <class Colour>
__device__ __forceinline__ int64_t blend_forward(const f32x2* __restrict__ uv, const f32x4* __restrict__ conic, const float* __restrict__ depth,
                                                 const int32_t* __restrict__ values, int64_t n, const GaussTile& tile, const Colour& colour,
                                                 f32x4* geom, f32x4* look, GaussPixel& acc) {
    int done = tile.inside ? 0 : 1;
    int64_t base = tile.start;
    for (; base < tile.end; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch has been read by every lane
        stage_batch(uv, conic, depth, values, n, tile, base, colour, geom, look);
        const int m = (int)(tile.end - base < BATCH ? tile.end - base : BATCH);
        for (int k = 0; k < m && !done; ++k) {
            const f32x4 a = geom[k], b = look[k];
            if (blend_step(a, b, tile.px, tile.py, acc.T, [&](const GaussBlend& s) { accumulate(acc, colour.at(k, b), b.w, s); })) {
                done = 1;
                break;
            }
        }
    }
    return (base < tile.end ? base : tile.end) - tile.start;
}

// The three images of a pixel that the image has.
__device__ __forceinline__ void store_images(const GaussTile& tile, int H, int W, const GaussPixel& acc, float* __restrict__ rgb,
                                             float* __restrict__ depth_out, float* __restrict__ alpha_out) {
    const int64_t plane = (int64_t)H * W, pix = (int64_t)tile.j * W + tile.i;
    float* out = rgb + tile.view * 3 * plane + pix;
    out[0] = dvd(acc.c0, 255.0f);
    out[plane] = dvd(acc.c1, 255.0f);
    out[2 * plane] = dvd(acc.c2, 255.0f);
    depth_out[tile.view * plane + pix] = acc.D;
    alpha_out[tile.view * plane + pix] = sub(1.0f, acc.T);
}

// The raw accumulators (C0, C1, C2, D, T) of a pixel that the image has, into state (V, 5, H, W): what a backward needs unrounded.
__device__ __forceinline__ void store_state(const GaussTile& tile, int H, int W, const GaussPixel& acc, float* __restrict__ state) {
    const int64_t plane = (int64_t)H * W;
    float* st = state + tile.view * 5 * plane + (int64_t)tile.j * W + tile.i;
    st[0] = acc.c0;
    st[plane] = acc.c1;
    st[2 * plane] = acc.c2;
    st[3 * plane] = acc.D;
    st[4 * plane] = acc.T;
}

// ------------------------------------------------------------------------------------------------ the blend's backward at a pixel (§24)
// What a pixel of the backward holds before its walk: the upstream gradients of the raw accumulators (colour over 255), gA T_final, and
// the forward's final accumulators; zeros for a lane the image does not have.
struct GaussUpstream {
    float gC0 = 0.0f, gC1 = 0.0f, gC2 = 0.0f, gD = 0.0f, gAT = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sD = 0.0f;
};

__device__ __forceinline__ GaussUpstream load_upstream(const GaussTile& tile, int H, int W, const float* __restrict__ state,
                                                       const float* __restrict__ d_rgb, const float* __restrict__ d_depth,
                                                       const float* __restrict__ d_alpha) {
    GaussUpstream u;
    if (tile.inside) {
        const int64_t plane = (int64_t)H * W, pix = (int64_t)tile.j * W + tile.i;
        const float* g = d_rgb + tile.view * 3 * plane + pix;
        u.gC0 = dvd(g[0], 255.0f);
        u.gC1 = dvd(g[plane], 255.0f);
        u.gC2 = dvd(g[2 * plane], 255.0f);
        u.gD = d_depth[tile.view * plane + pix];
        const float* st = state + tile.view * 5 * plane + pix;
        u.s0 = st[0]; u.s1 = st[plane]; u.s2 = st[2 * plane]; u.sD = st[3 * plane];
        u.gAT = mul(d_alpha[tile.view * plane + pix], st[4 * plane]);      // gA T_final
    }
    return u;
}

// A blended entry's four sums that need no alpha gradient: the colour's and the depth's.
__device__ __forceinline__ void blend_bwd_direct(const GaussUpstream& u, const GaussBlend& s, float (&r)[GAUSS_SUMS]) {
    r[SUM_COLOUR] = mul(u.gC0, s.w);
    r[SUM_COLOUR + 1] = mul(u.gC1, s.w);
    r[SUM_COLOUR + 2] = mul(u.gC2, s.w);
    r[SUM_ZC] = mul(u.gD, s.w);
}

// own: what the entry itself adds to the loss per unit of w; behind: what everything behind it adds.  acc: after the entry was added.
__device__ __forceinline__ float blend_bwd_own(const GaussUpstream& u, const f32x4& c, float zc) {
    return add(add(add(mul(u.gC0, c.x), mul(u.gC1, c.y)), mul(u.gC2, c.z)), mul(u.gD, zc));
}

__device__ __forceinline__ float blend_bwd_behind(const GaussUpstream& u, const GaussPixel& acc) {
    return add(add(add(mul(u.gC0, sub(u.s0, acc.c0)), mul(u.gC1, sub(u.s1, acc.c1))), mul(u.gC2, sub(u.s2, acc.c2))),
               mul(u.gD, sub(u.sD, acc.D)));
}

// The six sums through alpha, for an entry whose alpha the cap did not take: a, b the staged entry, T the transmittance before it.
__device__ __forceinline__ void blend_bwd_alpha(const GaussUpstream& u, const f32x4& a, const f32x4& b, const GaussBlend& s, float T, float own,
                                                float behind, float (&r)[GAUSS_SUMS]) {
    const float dal = add(sub(mul(T, own), dvd(behind, s.om)), dvd(u.gAT, s.om));
    r[SUM_OPACITY] = mul(dal, s.ge);
    const float dp = mul(mul(dal, b.y), s.ge);
    r[SUM_A] = mul(dp, mul(-0.5f, mul(s.dx, s.dx)));
    r[SUM_B] = mul(dp, -mul(s.dx, s.dy));
    r[SUM_C] = mul(dp, mul(-0.5f, mul(s.dy, s.dy)));
    r[SUM_U] = mul(dp, -add(mul(a.z, s.dx), mul(a.w, s.dy)));
    r[SUM_V] = mul(dp, -add(mul(b.x, s.dy), mul(a.w, s.dx)));
}

// ------------------------------------------------------------------------------------------------ partials and reductions (§24)
// Columns [C0, C0 + N) of the partials of (view, Gaussian) o, rows [off, off + count) of the (E, GAUSS_SUMS) buffer in the order the
// forward wrote its entries, added in ascending order from +0.0 and handed to then(acc).  Nothing is read and then does not run where
// the Gaussian was dropped in the view or the offset is not one of this call's entries.
template <int C0, int N, class Then>
__device__ __forceinline__ void with_partials(const float* __restrict__ partial, const int32_t* __restrict__ count,
                                              const int64_t* __restrict__ offsets, int64_t o, int64_t E, Then&& then) {
    const int cnt = count[o];
    if (cnt <= 0) return;
    const int64_t off = offsets[o];
    if (off < 0 || off > E - cnt) return;
    float acc[N];
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = 0.0f;
    for (int k = 0; k < cnt; ++k) {
        const float* row = partial + (off + k) * GAUSS_SUMS + C0;
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = add(acc[c], row[c]);
    }
    then(acc);
}

// The fixed order of every sum over a tile's 256 lanes: an xor butterfly inside each wave (addition commutes, so every lane of the wave
// ends with the same bits), then the four waves as ((w0 + w1) + w2) + w3.  The butterfly runs over 1, 2, 4, ... 32: it is not common.h's
// wave_sum, which starts at 32 and rounds differently.
__device__ __forceinline__ float plus(float a, float b) { return add(a, b); }
__device__ __forceinline__ double plus(double a, double b) { return a + b; }
__device__ __forceinline__ int plus(int a, int b) { return a + b; }
__device__ __forceinline__ long long plus(long long a, long long b) { return a + b; }

template <class T>
__device__ __forceinline__ T butterfly_sum(T r) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) r = plus(r, __shfl_xor(r, s));
    return r;
}

template <class T>
__device__ __forceinline__ T four_waves(T w0, T w1, T w2, T w3) { return plus(plus(plus(w0, w1), w2), w3); }

// ------------------------------------------------------------------------------------------------ one view's chain rule (§24)
// The sums `acc` of a (view, Gaussian)'s partials through the projection `w` = gauss_view(m, ...): what reaches xc, yc, zc (dzc with the
// path through the Jacobian, a clamped tx or ty passing nothing through xc / zc), the rows of T = J R, and the view's addend to the
// covariance's gradient in the order (xx, xy, xz, yy, yz, zz), off-diagonal entries with both halves.
struct GaussViewBwd {
    float dxc, dyc, dzc, dt0[3], dt1[3], dcov[6];
};

__device__ __forceinline__ void gauss_view_bwd(const float* __restrict__ m, const GaussView& w, const GaussCam& cam,
                                               const float (&acc)[GAUSS_SUMS], GaussViewBwd& o) {
    const float A = dvd(w.c, w.det), B = -dvd(w.b, w.det), C = dvd(w.a, w.det);
    // conic -> (a, b, c): with K the conic and G = [[gA, gB / 2], [gB / 2, gC]], d(a, b, c) = -(K G K) read as (00, 2 x 01, 11)
    const float gA = acc[SUM_A], hB = mul(0.5f, acc[SUM_B]), gC = acc[SUM_C];
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
            if (r == k)
                o.dcov[e] = add(add(mul(da, mul(w.t0[r], w.t0[r])), mul(db, mul(w.t0[r], w.t1[r]))), mul(dc, mul(w.t1[r], w.t1[r])));
            else
                o.dcov[e] = add(add(mul(da2, mul(w.t0[r], w.t0[k])), mul(db, add(mul(w.t0[r], w.t1[k]), mul(w.t0[k], w.t1[r])))),
                                mul(dc2, mul(w.t1[r], w.t1[k])));
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.dt0[k] = add(mul(da2, w.v0[k]), mul(db, w.v1[k]));
        o.dt1[k] = add(mul(dc2, w.v1[k]), mul(db, w.v0[k]));
    }
    // T -> j00, j02, j11, j12
    const float dj00 = add(add(mul(o.dt0[0], m[0]), mul(o.dt0[1], m[1])), mul(o.dt0[2], m[2]));
    const float dj02 = add(add(mul(o.dt0[0], m[8]), mul(o.dt0[1], m[9])), mul(o.dt0[2], m[10]));
    const float dj11 = add(add(mul(o.dt1[0], m[4]), mul(o.dt1[1], m[5])), mul(o.dt1[2], m[6]));
    const float dj12 = add(add(mul(o.dt1[0], m[8]), mul(o.dt1[1], m[9])), mul(o.dt1[2], m[10]));
    // j -> xc, yc, zc
    const float dtx = -dvd(mul(dj02, cam.fx), w.zz), dty = -dvd(mul(dj12, cam.fy), w.zz);
    const float dzz = -add(dvd(mul(dj02, w.j02), w.zz), dvd(mul(dj12, w.j12), w.zz));
    float dzc = acc[SUM_ZC];                                                // the depth term
    dzc = sub(dzc, dvd(mul(dj00, w.j00), w.zc));
    dzc = sub(dzc, dvd(mul(dj11, w.j11), w.zc));
    dzc = add(dzc, mul(mul(2.0f, w.zc), dzz));
    dzc = add(dzc, mul(dtx, w.kx));
    dzc = add(dzc, mul(dty, w.ky));
    float dqx = mul(acc[SUM_U], cam.fx), dqy = mul(acc[SUM_V], cam.fy);
    if (w.kx == w.qx) dqx = add(dqx, mul(dtx, w.zc));                       // a clamped tx passes nothing through xc / zc
    if (w.ky == w.qy) dqy = add(dqy, mul(dty, w.zc));
    o.dxc = dvd(dqx, w.zc); o.dyc = dvd(dqy, w.zc);
    dzc = sub(dzc, dvd(mul(dqx, w.qx), w.zc));
    dzc = sub(dzc, dvd(mul(dqy, w.qy), w.zc));
    o.dzc = dzc;
}

// ------------------------------------------------------------------------------------------------ a sum over all Gaussians (§28)
// The gradient of a view's matrices sums over every Gaussian that goes through the matrix.  A workgroup of 256 lanes owns chunk
// blockIdx.x of 256 consecutive Gaussians in view blockIdx.y; a lane holds POSE_SUMS values g, its matrix id and whether it takes part.
// Per id present among the lanes that take part, smallest first, the 256 values (+0.0 for a lane that holds another id or takes no
// part) go through the tile's order (butterfly_sum, four_waves) and are stored plainly at stage[view][id][chunk]; the entry point has
// zeroed stage (view, nmat, chunks, POSE_SUMS), so an id absent from a chunk reads as +0.0.  pose_finish then adds a (view, matrix)'s chunks.
constexpr int POSE_SUMS = 12;

struct PoseScratch {                                // LDS
    float wsum[4 * POSE_SUMS];
    int least[4];
};

__device__ __forceinline__ void pose_reduce_one(const float (&g)[POSE_SUMS], bool mine, float* __restrict__ out, PoseScratch& lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < POSE_SUMS; ++c) {
        const float r = butterfly_sum(mine ? g[c] : 0.0f);
        if (lane == 0) lds.wsum[wave * POSE_SUMS + c] = r;
    }
    __syncthreads();
    if (threadIdx.x < POSE_SUMS) {
        const float* w = lds.wsum + threadIdx.x;
        out[threadIdx.x] = four_waves(w[0], w[POSE_SUMS], w[2 * POSE_SUMS], w[3 * POSE_SUMS]);
    }
    __syncthreads();                                                        // wsum may be written again
}

// stage_view: the view's (nmat, chunks, POSE_SUMS) piece.  Every lane of the workgroup calls it.
__device__ __forceinline__ void pose_reduce(const float (&g)[POSE_SUMS], bool takes_part, int id, int nmat, float* __restrict__ stage_view,
                                            int64_t chunks, PoseScratch& lds) {
    if (nmat == 1) {
        if (__syncthreads_or(takes_part)) pose_reduce_one(g, takes_part, stage_view + (int64_t)blockIdx.x * POSE_SUMS, lds);
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int prev = -1;;) {                                                 // the ids present, ascending; absent ones are skipped
        int cur = takes_part && id > prev ? id : 0x7fffffff;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) cur = min(cur, __shfl_xor(cur, s));
        if (lane == 0) lds.least[wave] = cur;
        __syncthreads();
        cur = min(min(lds.least[0], lds.least[1]), min(lds.least[2], lds.least[3]));
        __syncthreads();                                                    // least may be written again
        if (cur == 0x7fffffff) return;                                      // the same for every lane
        pose_reduce_one(g, takes_part && id == cur, stage_view + ((int64_t)cur * chunks + blockIdx.x) * POSE_SUMS, lds);
        prev = cur;
    }
}

// Workgroup (matrix, view): lane l adds chunks l, l + 256, ... in ascending order from +0.0, the 256 lane sums go through the tile's
// order, and d_mats[view][matrix] is overwritten.  A template only so that the translation units that never launch it do not carry it.
template <int N>
__global__ __launch_bounds__(256) void pose_finish_kernel(const float* __restrict__ stage, int64_t chunks, float* __restrict__ d_mats) {
    __shared__ float wsum[4 * N];
    const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;       // view nmat + matrix
    const float* src = stage + row * chunks * N;
    float acc[N];
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = 0.0f;
    for (int64_t k = threadIdx.x; k < chunks; k += 256) {
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = add(acc[c], src[k * N + c]);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const float r = butterfly_sum(acc[c]);
        if (lane == 0) wsum[wave * N + c] = r;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const float* w = wsum + threadIdx.x;
        d_mats[row * N + threadIdx.x] = four_waves(w[0], w[N], w[2 * N], w[3 * N]);
    }
}

// ------------------------------------------------------------------------------------------------ what the entry points check
inline bool grid_ok(int64_t lanes) { return (lanes + 255) / 256 <= 0x7fffffffLL; }
inline bool entries_ok(int64_t E) { return E >= 1 && E <= 0x7fffffffLL; }

// the tile grid of an H x W image
struct GaussGrid {
    int TX, TY, NT;
    __host__ __device__ GaussGrid(int H, int W) : TX((W + TILE - 1) / TILE), TY((H + TILE - 1) / TILE), NT(TX * TY) {}
};

// the image and the tile grid shared by every entry point: V NT < 2^31
inline int check_views(const char* name, int64_t n, int V, int H, int W) {
    MUDG_REQUIRE(n > 0 && V > 0, "%s: %lld Gaussians in %d views", name, (long long)n, V);
    MUDG_REQUIRE(n <= 0x7fffffffLL, "%s: %lld Gaussians (the sorted value is a 32-bit index)", name, (long long)n);
    MUDG_REQUIRE(H > 0 && W > 0 && splat_args_ok(H, W), "%s: a %d x %d image", name, H, W);
    const int64_t NT = GaussGrid(H, W).NT;
    MUDG_REQUIRE((int64_t)V * NT < (1LL << 31), "%s: %d views of %lld tiles (V NT < 2^31)", name, V, (long long)NT);
    return MUDG_OK;
}

// the depth range and the intrinsics; why: what the caller's message adds about the depth range
inline int check_camera(const char* name, float fx, float fy, float cx, float cy, float znear, float zfar, const char* why = "") {
    MUDG_REQUIRE(std::isfinite(znear) && std::isfinite(zfar) && znear > 0.0f && zfar > znear, "%s: need finite 0 < znear < zfar%s", name, why);
    MUDG_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0f && fy > 0.0f && std::isfinite(cx) && std::isfinite(cy),
                 "%s: intrinsics %g %g %g %g", name, (double)fx, (double)fy, (double)cx, (double)cy);
    return MUDG_OK;
}

// §28: the stage buffer of a pose gradient, (V, nmat, ceil(n / 256), POSE_SUMS) floats, cleared; then, after the caller's kernel has
// stored the chunk sums, the finishing launch.
__host__ __device__ inline int64_t pose_chunks(int64_t n) { return (n + 255) / 256; }

inline bool pose_clear(float* stage, int64_t n, int V, int nmat, hipStream_t s) {
    return hipMemsetAsync(stage, 0, (size_t)V * nmat * pose_chunks(n) * POSE_SUMS * sizeof(float), s) == hipSuccess;
}

template <int N = POSE_SUMS>                        // a template for the kernel's reason: instantiated where it is called
inline void pose_finish(const float* stage, int64_t n, int V, int nmat, float* d_mats, hipStream_t s) {
    hipLaunchKernelGGL(pose_finish_kernel<N>, dim3((unsigned)nmat, (unsigned)V), dim3(256), 0, s, stage, pose_chunks(n), d_mats);
}
