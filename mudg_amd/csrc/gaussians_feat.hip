// gaussians_feat.hip — semantic Gaussians: every Gaussian carries a row of F feature values (class scores, 1 <= F <= 32)
// that is blended with its colour in the same walk over a tile, differentiated, and fitted with a softmax cross-entropy loss.
//   gauss_blend_feat      gauss_blend_train (§24) with one more line per blended entry: Fk += feat[g][k] w.  rgb, depth, alpha and state
//                         are its bits; feat_out (V, F, H, W) is the raw sum, its own state
//   gauss_blend_bwd_feat  gauss_blend_bwd (§24) with the features' share of `own` and `behind`.  What lies behind an entry in the feature
//                         channels is one scalar per pixel: Stot - P, the total sum_k gF_k F_k less the running prefix, so a pixel keeps
//                         F + 2 registers for the features.  The ten sums go to partial, the F sums gF_k w to partial_feat, both through the
//                         fixed order of §24.  Entries are reduced in sub-batches of 32 so that the four waves' sums stay below 64 KiB of
//                         LDS; the staging size changes no pixel's arithmetic
//   gauss_feat_bwd        a lane owns one (Gaussian, channel): per view the Gaussian's rows of partial_feat in ascending order from +0,
//                         the views added in order
//   gauss_class_loss      a workgroup owns a tile, a lane a pixel: the softmax of the pixel's F values with the polynomial exponential of
//                         §23 and the polynomial logarithm below, the map e_k / S - [k == label], and the tile's sums of the loss and of
//                         the labelled pixels in §24's order.  _finish adds the tiles in one workgroup; _bwd scales the maps
// F is a template bound (4, 8, 16, 24, 32); the runtime F cuts the loads and stores, and the padded columns hold +0.0, which changes no
// sum.  Everything is fp32, each operation a single rounded one in the order DESIGN.md §29 writes it, so every output is bit-equal to
// the numpy definition in tests/gaussians_feat_reference.py and a repeat run gives the same bits.  No atomics.  No MFMA operand is touched.
#include "depth_shared.h"
#include "gauss_shared.h"

#include <type_traits>

namespace {

constexpr int FEAT_MAX = 32;
constexpr int SUB = 32;                             // entries of a batch whose sums the backward reduces at a time
constexpr float MIN_SCORE = -80.0f;                 // x_k - max below this is this: E stays a normal number
constexpr int LOSS_COLS = 2;                        // a tile's partial: sum l, the labelled count (int32 bits)

// L(s) for 1 <= s <= 32: s = 2^e m with sqrt(1/2) <= m < sqrt(2) (frexp, and one exact doubling), t = m - 1 (exact), log(1 + t) = t P(t)
// with P of degree 8 in Horner form, and e ln 2 added last.  L(1) is exactly +0.0.
__device__ __forceinline__ float gauss_log(float s) {
    int e;
    float m = frexpf(s, &e);                        // [0.5, 1)
    if (m < 0x1.6a09e6p-1f) { m = mul(m, 2.0f); e -= 1; }
    const float t = sub(m, 1.0f);
    float r = 0x1.6626eap-4f;
    r = add(mul(r, t), -0x1.26729ep-3f);
    r = add(mul(r, t), 0x1.322850p-3f);
    r = add(mul(r, t), -0x1.5329bep-3f);
    r = add(mul(r, t), 0x1.98b80ap-3f);
    r = add(mul(r, t), -0x1.0005a6p-2f);
    r = add(mul(r, t), 0x1.555790p-2f);
    r = add(mul(r, t), -0x1.fffff8p-2f);
    r = add(mul(r, t), 1.0f);
    return add(mul((float)e, 0x1.62e430p-1f), mul(r, t));
}

// The feature rows of the tile's sorted entries [base, base + count) into LDS rows of FB floats: +0.0 in the columns from F on, past
// the tile's end and for a sorted value outside the cloud, whose row is never read.  The caller's barrier follows.
template <int FB>
__device__ __forceinline__ void stage_features(const float* __restrict__ feat, int F, const int32_t* __restrict__ values, int64_t n,
                                               const GaussTile& tile, int64_t base, int count, float* rows) {
    for (int idx = threadIdx.x; idx < count * FB; idx += 256) {
        const int e = idx / FB, k = idx - e * FB;
        float v = 0.0f;
        if (k < F && base + e < tile.end) {
            const int64_t g = values[base + e];
            if (g >= 0 && g < n) v = feat[g * F + k];
        }
        rows[idx] = v;
    }
}

template <int FB>
__global__ __launch_bounds__(256) void gauss_blend_feat_kernel(const float* __restrict__ colour, int64_t per_view, const float* __restrict__ feat,
                                                                int F, const f32x2* __restrict__ uv, const f32x4* __restrict__ conic,
                                                                const float* __restrict__ depth, const int32_t* __restrict__ values,
                                                                const int32_t* __restrict__ ranges, int64_t n, int64_t E, int TX, int NT, int H,
                                                                int W, float* __restrict__ rgb, float* __restrict__ depth_out,
                                                                float* __restrict__ alpha_out, float* __restrict__ feat_out,
                                                                float* __restrict__ state) {
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    __shared__ f32x4 tint[BATCH];
    __shared__ __attribute__((aligned(16))) float rows[BATCH * FB];
    const GaussTile tile = gauss_tile(blockIdx.x, ranges, E, TX, NT, H, W);
    const FloatColour tints = {colour + tile.view * per_view, tint};
    GaussPixel acc;
    float Fk[FB];
#pragma unroll
    for (int c = 0; c < FB; ++c) Fk[c] = 0.0f;
    int done = tile.inside ? 0 : 1;
    for (int64_t base = tile.start; base < tile.end; base += BATCH) {      // blend_forward's loop (gauss_shared.h) with the features' line
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch has been read by every lane
        const int m = (int)(tile.end - base < BATCH ? tile.end - base : BATCH);
        stage_features<FB>(feat, F, values, n, tile, base, m, rows);
        stage_batch(uv, conic, depth, values, n, tile, base, tints, geom, look);
        for (int k = 0; k < m && !done; ++k) {
            const f32x4 a = geom[k], b = look[k];
            if (blend_step(a, b, tile.px, tile.py, acc.T, [&](const GaussBlend& s) {
                    accumulate(acc, tints.at(k, b), b.w, s);
                    const float* f = rows + k * FB;
#pragma unroll
                    for (int c = 0; c < FB; ++c) Fk[c] = add(Fk[c], mul(f[c], s.w));
                })) {
                done = 1;
                break;
            }
        }
    }
    if (tile.inside) {
        store_images(tile, H, W, acc, rgb, depth_out, alpha_out);
        if (state) store_state(tile, H, W, acc, state);                    // NULL: inference
        const int64_t plane = (int64_t)H * W;
        float* out = feat_out + tile.view * F * plane + (int64_t)tile.j * W + tile.i;
#pragma unroll
        for (int c = 0; c < FB; ++c)
            if (c < F) out[c * plane] = Fk[c];
    }
}

// order[e] as in gauss_blend_bwd: a value outside [0, E) writes nothing; the batches never staged keep the entry point's zeros.
template <int FB>
__global__ __launch_bounds__(256) void gauss_blend_bwd_feat_kernel(
    const float* __restrict__ colour, int64_t per_view, const float* __restrict__ feat, int F, const f32x2* __restrict__ uv,
    const f32x4* __restrict__ conic, const float* __restrict__ depth, const int32_t* __restrict__ values, const int64_t* __restrict__ order,
    const int32_t* __restrict__ ranges, int64_t n, int64_t E, int TX, int NT, int H, int W, const float* __restrict__ state,
    const float* __restrict__ feat_out, const float* __restrict__ d_rgb, const float* __restrict__ d_depth, const float* __restrict__ d_alpha,
    const float* __restrict__ d_feat, float* __restrict__ partial, float* __restrict__ partial_feat) {
    constexpr int COLS = GAUSS_SUMS + FB;
    __shared__ f32x4 geom[BATCH];
    __shared__ f32x4 look[BATCH];
    __shared__ f32x4 tint[BATCH];
    __shared__ __attribute__((aligned(16))) float rows[SUB * FB];
    __shared__ float wsum[4 * SUB * COLS];                                  // the four waves' sums of every entry of the sub-batch
    const GaussTile tile = gauss_tile(blockIdx.x, ranges, E, TX, NT, H, W);
    const FloatColour tints = {colour + tile.view * per_view, tint};
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const GaussUpstream up = load_upstream(tile, H, W, state, d_rgb, d_depth, d_alpha);
    float gF[FB], Stot = 0.0f, P = 0.0f;                                    // sum_k gF_k F_k: the whole pixel's, and the entries' so far
#pragma unroll
    for (int c = 0; c < FB; ++c) gF[c] = 0.0f;
    if (tile.inside) {
        const int64_t plane = (int64_t)H * W, pix = tile.view * F * plane + (int64_t)tile.j * W + tile.i;
#pragma unroll
        for (int c = 0; c < FB; ++c) {
            if (c < F) {
                gF[c] = d_feat[pix + c * plane];
                Stot = add(Stot, mul(gF[c], feat_out[pix + c * plane]));
            }
        }
    }
    GaussPixel acc;
    int done = tile.inside ? 0 : 1;
    for (int64_t base = tile.start; base < tile.end; base += BATCH) {
        if (__syncthreads_count(done) == 256) break;                        // also: the last batch has been read
        stage_batch(uv, conic, depth, values, n, tile, base, tints, geom, look);
        const int m = (int)(tile.end - base < BATCH ? tile.end - base : BATCH);
        for (int part = 0; part < m; part += SUB) {
            const int ms = m - part < SUB ? m - part : SUB;
            stage_features<FB>(feat, F, values, n, tile, base + part, ms, rows);
            __syncthreads();                                                // also: the last sub-batch's sums have been read
            for (int k = 0; k < ms; ++k) {                                  // every lane walks every entry: the reduction needs them all
                float r[GAUSS_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                float w = 0.0f;
                bool blends = false;
                if (!done) {
                    const f32x4 a = geom[part + k], b = look[part + k];
                    done = blend_step(a, b, tile.px, tile.py, acc.T, [&](const GaussBlend& s) {
                        blends = true;
                        w = s.w;
                        const f32x4 c = tints.at(part + k, b);
                        const float T = acc.T, zc = b.w;
                        accumulate(acc, c, zc, s);
                        const float* f = rows + k * FB;
                        float dot = 0.0f;                                   // sum_k gF_k feat[g][k]
#pragma unroll
                        for (int q = 0; q < FB; ++q) dot = add(dot, mul(gF[q], f[q]));
                        P = add(P, mul(dot, s.w));
                        blend_bwd_direct(up, s, r);
                        if (s.raw > MAX_ALPHA) return;                      // the cap passes no gradient
                        const float own = add(blend_bwd_own(up, c, zc), dot);
                        const float behind = add(blend_bwd_behind(up, acc), sub(Stot, P));
                        blend_bwd_alpha(up, a, b, s, T, own, behind, r);
                    });
                }
                float* out = wsum + ((size_t)wave * SUB + k) * COLS;
                if (__ballot(blends) != 0) {
#pragma unroll
                    for (int c = 0; c < GAUSS_SUMS; ++c) {
                        const float v = butterfly_sum(r[c]);
                        if (lane == 0) out[c] = v;
                    }
#pragma unroll
                    for (int c = 0; c < FB; ++c) {
                        const float v = butterfly_sum(blends ? mul(gF[c], w) : 0.0f);
                        if (lane == 0) out[GAUSS_SUMS + c] = v;
                    }
                } else if (lane == 0) {                                     // sixty-four times +0.0 is +0.0
#pragma unroll
                    for (int c = 0; c < COLS; ++c) out[c] = 0.0f;
                }
            }
            __syncthreads();
            for (int idx = threadIdx.x; idx < ms * COLS; idx += 256) {
                const int e = idx / COLS, c = idx - e * COLS;
                if (c >= GAUSS_SUMS + F) continue;
                const int64_t at = order[base + part + e];
                if (at < 0 || at >= E) continue;
                const float* v = wsum + idx;
                const float sum = four_waves(v[0], v[SUB * COLS], v[2 * SUB * COLS], v[3 * SUB * COLS]);
                if (c < GAUSS_SUMS) partial[at * GAUSS_SUMS + c] = sum;
                else partial_feat[at * F + (c - GAUSS_SUMS)] = sum;
            }
        }
    }
}

__global__ __launch_bounds__(256) void gauss_feat_bwd_kernel(const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                              const float* __restrict__ partial_feat, int64_t E, int64_t n, int V, int F,
                                                              float* __restrict__ d_feat_g) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * F) return;
    const int64_t g = idx / F;
    const int k = (int)(idx - g * F);
    float total = 0.0f;
    for (int view = 0; view < V; ++view) {                                  // with_partials' guards (gauss_shared.h), on rows of F
        const int64_t o = (int64_t)view * n + g;
        const int cnt = count[o];
        if (cnt <= 0) continue;
        const int64_t off = offsets[o];
        if (off < 0 || off > E - cnt) continue;
        float acc = 0.0f;
        for (int j = 0; j < cnt; ++j) acc = add(acc, partial_feat[(off + j) * F + k]);
        total = add(total, acc);
    }
    d_feat_g[idx] = total;
}

template <int FB>
__global__ __launch_bounds__(256) void gauss_class_loss_kernel(const float* __restrict__ x, const uint8_t* __restrict__ labels, int F, int TX,
                                                                int NT, int H, int W, float* __restrict__ maps, float* __restrict__ partial) {
    __shared__ float wl[4];
    __shared__ int wc[4];
    const TileId id = tile_id(blockIdx.x, TX, NT);
    const int i = id.ti * TILE + (threadIdx.x & (TILE - 1)), j = id.tj * TILE + (threadIdx.x >> 4);
    float l = 0.0f;                                                         // a lane outside the image, or unlabelled, adds +0.0
    int cnt = 0;
    if (i < W && j < H) {
        const int64_t plane = (int64_t)H * W, pix = (int64_t)j * W + i;
        const int label = labels[id.group * plane + pix];
        const float* in = x + id.group * F * plane + pix;
        float* out = maps + id.group * F * plane + pix;
        if (label < F) {
            float v[FB];
            float m = in[0];
#pragma unroll
            for (int k = 0; k < FB; ++k) v[k] = k < F ? in[k * plane] : 0.0f;
#pragma unroll
            for (int k = 1; k < FB; ++k)
                if (k < F) m = fmaxf(m, v[k]);
            float S = 0.0f, pl = 0.0f;
#pragma unroll
            for (int k = 0; k < FB; ++k) {
                if (k < F) {
                    const float p = fmaxf(sub(v[k], m), MIN_SCORE);
                    v[k] = gauss_exp(p);
                    S = add(S, v[k]);
                    if (k == label) pl = p;
                }
            }
#pragma unroll
            for (int k = 0; k < FB; ++k)
                if (k < F) out[k * plane] = sub(dvd(v[k], S), k == label ? 1.0f : 0.0f);
            l = sub(gauss_log(S), pl);
            cnt = 1;
        } else {
            for (int k = 0; k < F; ++k) out[k * plane] = 0.0f;
        }
    }
    l = butterfly_sum(l);
    cnt = butterfly_sum(cnt);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wl[wave] = l; wc[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[(int64_t)blockIdx.x * LOSS_COLS] = four_waves(wl[0], wl[1], wl[2], wl[3]);
        partial[(int64_t)blockIdx.x * LOSS_COLS + 1] = __int_as_float(four_waves(wc[0], wc[1], wc[2], wc[3]));
    }
}

// One workgroup: lane l adds the tiles l, l + 256, ... in ascending order in fp64 (the count in int64), the butterfly and the wave order
// combine the lanes, lane 0 writes totals = (sum l, the count as int32 bits, float(max(count, 1)), the loss).
__global__ __launch_bounds__(256) void gauss_class_loss_finish_kernel(const float* __restrict__ partial, int64_t P, float weight,
                                                                       float* __restrict__ totals) {
    __shared__ double wreal[4];
    __shared__ long long wcount[4];
    double sum = 0.0;
    long long cnt = 0;
    for (int64_t p = threadIdx.x; p < P; p += 256) {
        sum += (double)partial[p * LOSS_COLS];
        cnt += (long long)__float_as_int(partial[p * LOSS_COLS + 1]);
    }
    sum = butterfly_sum(sum);
    cnt = butterfly_sum(cnt);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wreal[wave] = sum; wcount[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double L = four_waves(wreal[0], wreal[1], wreal[2], wreal[3]);
        const long long count = four_waves(wcount[0], wcount[1], wcount[2], wcount[3]);
        const long long seen = count < 1 ? 1 : count;
        totals[0] = (float)L;
        totals[1] = __int_as_float((int)(count > 0x7fffffffLL ? 0x7fffffffLL : count));
        totals[2] = (float)seen;
        totals[3] = mul(weight, (float)(L / (double)seen));
    }
}

__global__ __launch_bounds__(256) void gauss_class_loss_bwd_kernel(const float* __restrict__ maps, const float* __restrict__ totals,
                                                                    const float* __restrict__ upstream, float weight, int64_t count,
                                                                    float* __restrict__ d_x) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    d_x[idx] = mul(dvd(mul(upstream[0], weight), totals[2]), maps[idx]);
}

// fn(std::integral_constant<int, FB>) for the smallest bound that holds F
template <class Fn>
inline void with_feature_bound(int F, Fn&& fn) {
    if (F <= 4) fn(std::integral_constant<int, 4>{});
    else if (F <= 8) fn(std::integral_constant<int, 8>{});
    else if (F <= 16) fn(std::integral_constant<int, 16>{});
    else if (F <= 24) fn(std::integral_constant<int, 24>{});
    else fn(std::integral_constant<int, FEAT_MAX>{});
}

inline int check_features(const char* name, int F, int colour_views) {
    MUDG_REQUIRE(F >= 1 && F <= FEAT_MAX, "%s: %d features (1 .. %d)", name, F, FEAT_MAX);
    MUDG_REQUIRE(colour_views == 0 || colour_views == 1, "%s: colour_views %d (0: colours (n, 3); 1: colours (V, n, 3))", name, colour_views);
    return MUDG_OK;
}

// the images of the class loss: V NT workgroups, V F H W values
inline int check_scores(const char* name, int V, int F, int H, int W) {
    MUDG_REQUIRE(F >= 1 && F <= FEAT_MAX, "%s: %d features (1 .. %d)", name, F, FEAT_MAX);
    MUDG_REQUIRE(V > 0 && H > 0 && W > 0, "%s: %d views of %d x %d", name, V, H, W);
    return check_views(name, 1, V, H, W);
}

inline int check_weight(const char* name, float weight) {
    MUDG_REQUIRE(std::isfinite(weight) && weight >= 0.0f, "%s: a weight of %g (finite, not negative)", name, (double)weight);
    return MUDG_OK;
}

}  // namespace

extern "C" int mudg_gauss_blend_feat(const float* colours, int colour_views, const float* feat, int F, const float* uv, const float* conic,
                                     const float* depth, const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H,
                                     int W, float* rgb, float* depth_out, float* alpha, float* feat_out, float* state, void* stream) {
    const char* name = "mudg_gauss_blend_feat";
    MUDG_REQUIRE(colours && feat && uv && conic && depth && values_sorted && ranges && rgb && depth_out && alpha && feat_out,
                 "%s: null argument", name);
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv), "%s: unaligned projections", name);
    if (const int e = check_features(name, F, colour_views)) return e;
    if (const int e = check_views(name, n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "%s: %lld entries (1 .. 2^31 - 1)", name, (long long)E);
    const GaussGrid grid(H, W);
    with_feature_bound(F, [&](auto bound) {
        hipLaunchKernelGGL(gauss_blend_feat_kernel<decltype(bound)::value>, dim3((unsigned)((int64_t)V * grid.NT)), dim3(256), 0,
                           reinterpret_cast<hipStream_t>(stream), colours, colour_views ? 3 * n : 0, feat, F, reinterpret_cast<const f32x2*>(uv),
                           reinterpret_cast<const f32x4*>(conic), depth, values_sorted, ranges, n, E, grid.TX, grid.NT, H, W, rgb, depth_out, alpha,
                           feat_out, state);
    });
    return mudg_check_launch(name);
}

extern "C" int mudg_gauss_blend_bwd_feat(const float* colours, int colour_views, const float* feat, int F, const float* uv, const float* conic,
                                         const float* depth, const int32_t* values_sorted, const int64_t* order, const int32_t* ranges, int64_t n,
                                         int64_t E, int V, int H, int W, const float* state, const float* feat_out, const float* d_rgb,
                                         const float* d_depth, const float* d_alpha, const float* d_feat, float* partial, float* partial_feat,
                                         void* stream) {
    const char* name = "mudg_gauss_blend_bwd_feat";
    MUDG_REQUIRE(colours && feat && uv && conic && depth && values_sorted && order && ranges && state && feat_out && d_rgb && d_depth && d_alpha &&
                     d_feat && partial && partial_feat,
                 "%s: null argument", name);
    MUDG_REQUIRE(aligned16(conic) && aligned8(uv) && aligned8(order), "%s: unaligned projections or order", name);
    if (const int e = check_features(name, F, colour_views)) return e;
    if (const int e = check_views(name, n, V, H, W)) return e;
    MUDG_REQUIRE(entries_ok(E), "%s: %lld entries (1 .. 2^31 - 1)", name, (long long)E);
    MUDG_REQUIRE(E * F < (1LL << 31), "%s: %lld entries of %d features (E F < 2^31)", name, (long long)E, F);
    const GaussGrid grid(H, W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(partial, 0, (size_t)E * GAUSS_SUMS * sizeof(float), s) != hipSuccess) return mudg_check_launch(name);
    if (hipMemsetAsync(partial_feat, 0, (size_t)E * F * sizeof(float), s) != hipSuccess) return mudg_check_launch(name);
    with_feature_bound(F, [&](auto bound) {
        hipLaunchKernelGGL(gauss_blend_bwd_feat_kernel<decltype(bound)::value>, dim3((unsigned)((int64_t)V * grid.NT)), dim3(256), 0, s, colours,
                           colour_views ? 3 * n : 0, feat, F, reinterpret_cast<const f32x2*>(uv), reinterpret_cast<const f32x4*>(conic), depth,
                           values_sorted, order, ranges, n, E, grid.TX, grid.NT, H, W, state, feat_out, d_rgb, d_depth, d_alpha, d_feat, partial,
                           partial_feat);
    });
    return mudg_check_launch(name);
}

extern "C" int mudg_gauss_feat_bwd(const int32_t* count, const int64_t* offsets, const float* partial_feat, int64_t E, int64_t n, int V, int F,
                                   float* d_feat_g, void* stream) {
    const char* name = "mudg_gauss_feat_bwd";
    MUDG_REQUIRE(count && offsets && partial_feat && d_feat_g, "%s: null argument", name);
    MUDG_REQUIRE(aligned8(offsets), "%s: unaligned offsets", name);
    MUDG_REQUIRE(F >= 1 && F <= FEAT_MAX, "%s: %d features (1 .. %d)", name, F, FEAT_MAX);
    MUDG_REQUIRE(n > 0 && n <= 0x7fffffffLL && V > 0, "%s: %lld Gaussians in %d views", name, (long long)n, V);
    MUDG_REQUIRE(grid_ok(n * F), "%s: %lld Gaussians of %d features are more workgroups than a grid holds", name, (long long)n, F);
    MUDG_REQUIRE(entries_ok(E), "%s: %lld entries (1 .. 2^31 - 1)", name, (long long)E);
    MUDG_REQUIRE(E * F < (1LL << 31), "%s: %lld entries of %d features (E F < 2^31)", name, (long long)E, F);
    hipLaunchKernelGGL(gauss_feat_bwd_kernel, dim3((unsigned)((n * F + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), count,
                       offsets, partial_feat, E, n, V, F, d_feat_g);
    return mudg_check_launch(name);
}

extern "C" int mudg_gauss_class_loss(const float* x, const uint8_t* labels, int V, int F, int H, int W, float* maps, float* partial,
                                     void* stream) {
    const char* name = "mudg_gauss_class_loss";
    MUDG_REQUIRE(x && labels && maps && partial, "%s: null argument", name);
    MUDG_REQUIRE(aligned4(x) && aligned4(maps) && aligned4(partial), "%s: unaligned argument", name);
    if (const int e = check_scores(name, V, F, H, W)) return e;
    const GaussGrid grid(H, W);
    with_feature_bound(F, [&](auto bound) {
        hipLaunchKernelGGL(gauss_class_loss_kernel<decltype(bound)::value>, dim3((unsigned)((int64_t)V * grid.NT)), dim3(256), 0,
                           reinterpret_cast<hipStream_t>(stream), x, labels, F, grid.TX, grid.NT, H, W, maps, partial);
    });
    return mudg_check_launch(name);
}

extern "C" int mudg_gauss_class_loss_finish(const float* partial, int V, int H, int W, float weight, float* totals, void* stream) {
    const char* name = "mudg_gauss_class_loss_finish";
    MUDG_REQUIRE(partial && totals, "%s: null argument", name);
    MUDG_REQUIRE(aligned4(partial) && aligned4(totals), "%s: unaligned argument", name);
    if (const int e = check_scores(name, V, 1, H, W)) return e;
    if (const int e = check_weight(name, weight)) return e;
    hipLaunchKernelGGL(gauss_class_loss_finish_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partial,
                       (int64_t)V * GaussGrid(H, W).NT, weight, totals);
    return mudg_check_launch(name);
}

extern "C" int mudg_gauss_class_loss_bwd(const float* maps, const float* totals, const float* up, float weight, int V, int F, int H, int W,
                                         float* d_x, void* stream) {
    const char* name = "mudg_gauss_class_loss_bwd";
    MUDG_REQUIRE(maps && totals && up && d_x, "%s: null argument", name);
    MUDG_REQUIRE(aligned4(maps) && aligned4(totals) && aligned4(up) && aligned4(d_x), "%s: unaligned argument", name);
    if (const int e = check_scores(name, V, F, H, W)) return e;
    if (const int e = check_weight(name, weight)) return e;
    const int64_t count = (int64_t)V * F * H * W;
    MUDG_REQUIRE(grid_ok(count), "%s: %lld values are more workgroups than a grid holds", name, (long long)count);
    hipLaunchKernelGGL(gauss_class_loss_bwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), maps,
                       totals, up, weight, count, d_x);
    return mudg_check_launch(name);
}
