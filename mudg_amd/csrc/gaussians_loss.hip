// gaussians_loss.hip — the image loss of the Gaussian fit: (1 - l) mean|x - y| + l (1 - mean SSIM) + depth_weight times
// the masked mean absolute depth difference, and its backward, without a torch element-wise chain or an autograd tape.
//   gauss_loss         a workgroup of 256 lanes owns a 16 x 16 tile of one channel of one view.  It stages the 26 x 26 apron of x and y
//                      in LDS (zeros outside the image), runs the horizontal and then the vertical pass of the 11-tap window for the five
//                      moments, evaluates S and its three derivative maps per pixel, and reduces |x - y|, S, the depth difference and the
//                      depth count over the tile in one fixed order: an xor butterfly inside each wave, the four waves through LDS as
//                      ((w0 + w1) + w2) + w3.  The tiles of channel 0 carry the depth term.  No atomics on global memory
//   gauss_loss_finish  one workgroup: lane l adds the partials l, l + 256, ... in ascending order in fp64 (the count in int64), the same
//                      butterfly and wave order combine the lanes, lane 0 writes the means, the count and the loss
//   gauss_loss_bwd     the same tiling: the apron of the three maps, the two passes, then the chain rule of §26 per pixel
// Everything on images is fp32, each operation a single rounded one in the order DESIGN.md §26 writes it, so every output is bit-equal to
// the numpy definition in tests/gaussians_loss_reference.py and a repeat run gives the same bits.  No address depends on a pixel value.
// No MFMA operand is touched.
#include "depth_shared.h"
#include "gauss_shared.h"

namespace {

constexpr int TAPS = 11, HALO = 5;
constexpr int APRON = TILE + 2 * HALO;              // 26
constexpr int MOMENTS = 5, MAPS = 3, COLS = 4;      // a partial's row: sum|x - y|, sum S, the depth sum, the depth count (int32 bits)
// the finish buffer, eight words: loss, mean|x - y|, mean S, depth mean, float(max(count, 1)), count (int32 bits), 0, 0
constexpr float C1 = 0.0001f, C2 = 0.0009f;         // 0.01^2 and 0.03^2

// ops.SSIM_WINDOW / 65536: every tap exact in fp32, the sum exactly 1
__device__ __forceinline__ float tap(int k) {
    constexpr float w[TAPS] = {67.0f / 65536.0f,    498.0f / 65536.0f,  2359.0f / 65536.0f, 7167.0f / 65536.0f,
                               13960.0f / 65536.0f, 17434.0f / 65536.0f, 13960.0f / 65536.0f, 7167.0f / 65536.0f,
                               2359.0f / 65536.0f,  498.0f / 65536.0f,  67.0f / 65536.0f};
    return w[k];
}

__device__ __forceinline__ float sgn(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// the apron of one plane around tile (ti, tj): zeros outside the image
__device__ __forceinline__ void stage_apron(const float* __restrict__ plane, int ti, int tj, int H, int W, float* __restrict__ lds) {
    for (int k = threadIdx.x; k < APRON * APRON; k += 256) {
        const int r = k / APRON, c = k - r * APRON;
        const int j = tj * TILE + r - HALO, i = ti * TILE + c - HALO;
        lds[k] = (i >= 0 && i < W && j >= 0 && j < H) ? plane[(int64_t)j * W + i] : 0.0f;
    }
}

// the vertical pass of the window at the lane's pixel (row, col) of the tile, over the N planes the horizontal pass left in LDS
template <int N>
__device__ __forceinline__ void window_vertical(const float (&rows)[N][APRON * TILE], int row, int col, float (&out)[N]) {
#pragma unroll
    for (int p = 0; p < N; ++p) out[p] = 0.0f;
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        const int k = (row + q) * TILE + col;
        const float w = tap(q);
#pragma unroll
        for (int p = 0; p < N; ++p) out[p] = add(out[p], mul(w, rows[p][k]));
    }
}

__global__ __launch_bounds__(256) void gauss_loss_kernel(const float* __restrict__ rgb, const float* __restrict__ targets,
                                                          const float* __restrict__ depth, const float* __restrict__ depth_targets, int TX,
                                                          int NT, int H, int W, float* __restrict__ maps, float* __restrict__ partial) {
    __shared__ float xs[APRON * APRON];
    __shared__ float ys[APRON * APRON];
    __shared__ float rows[MOMENTS][APRON * TILE];                           // the horizontal pass: 26 rows of 16 columns
    __shared__ float wsum[4][COLS];
    const int64_t t = blockIdx.x;
    const TileId id = tile_id(t, TX, NT);
    const int64_t vc = id.group;                                            // view * 3 + channel
    const int ti = id.ti, tj = id.tj;
    const int64_t plane = (int64_t)H * W;
    stage_apron(rgb + vc * plane, ti, tj, H, W, xs);
    stage_apron(targets + vc * plane, ti, tj, H, W, ys);
    __syncthreads();
    for (int k = threadIdx.x; k < APRON * TILE; k += 256) {
        const int r = k >> 4, c = k & (TILE - 1);
        float a = 0.0f, m = 0.0f, b = 0.0f, n = 0.0f, cc = 0.0f;
#pragma unroll
        for (int q = 0; q < TAPS; ++q) {
            const float x = xs[r * APRON + c + q], y = ys[r * APRON + c + q], w = tap(q);
            a = add(a, mul(w, x));
            m = add(m, mul(w, y));
            b = add(b, mul(w, mul(x, x)));
            n = add(n, mul(w, mul(y, y)));
            cc = add(cc, mul(w, mul(x, y)));
        }
        rows[0][k] = a; rows[1][k] = m; rows[2][k] = b; rows[3][k] = n; rows[4][k] = cc;
    }
    __syncthreads();
    const int col = threadIdx.x & (TILE - 1), row = threadIdx.x >> 4;
    const int i = ti * TILE + col, j = tj * TILE + row;
    const bool inside = i < W && j < H;
    float mom[MOMENTS];
    window_vertical(rows, row, col, mom);
    const float a = mom[0], m = mom[1], b = mom[2], n = mom[3], c = mom[4];
    const float aa = mul(a, a), mm = mul(m, m), am = mul(a, m);
    const float s1 = sub(b, aa), s2 = sub(n, mm), s12 = sub(c, am);
    const float A1 = add(mul(2.0f, am), C1), A2 = add(mul(2.0f, s12), C2);
    const float B1 = add(add(aa, mm), C1), B2 = add(add(s1, s2), C2);
    const float den = mul(B1, B2);
    const float S = dvd(mul(A1, A2), den);
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;                                  // a lane outside the image adds +0.0
    int r3 = 0;
    if (inside) {
        const int64_t pix = (int64_t)j * W + i;
        float* out = maps + vc * MAPS * plane + pix;
        out[0] = dvd(add(mul(mul(2.0f, m), sub(A2, A1)), mul(mul(mul(2.0f, a), S), sub(B1, B2))), den);      // Dm
        out[plane] = -dvd(S, B2);                                                                              // Ds1
        out[2 * plane] = dvd(mul(2.0f, A1), den);                                                              // Ds12
        r0 = fabsf(sub(xs[(row + HALO) * APRON + col + HALO], ys[(row + HALO) * APRON + col + HALO]));
        r1 = S;
        if (depth && vc % 3 == 0) {
            const int64_t o = (vc / 3) * plane + pix;
            const float want = depth_targets[o];
            if (want > 0.0f) {
                r2 = fabsf(sub(depth[o], want));
                r3 = 1;
            }
        }
    }
    r0 = butterfly_sum(r0);
    r1 = butterfly_sum(r1);
    r2 = butterfly_sum(r2);
    r3 = butterfly_sum(r3);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wsum[wave][0] = r0; wsum[wave][1] = r1; wsum[wave][2] = r2; wsum[wave][3] = __int_as_float(r3);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        partial[t * COLS + k] = four_waves(wsum[0][k], wsum[1][k], wsum[2][k], wsum[3][k]);
    } else if (threadIdx.x == 3) {
        const int cnt = four_waves(__float_as_int(wsum[0][3]), __float_as_int(wsum[1][3]), __float_as_int(wsum[2][3]), __float_as_int(wsum[3][3]));
        partial[t * COLS + 3] = __int_as_float(cnt);
    }
}

__global__ __launch_bounds__(256) void gauss_loss_finish_kernel(const float* __restrict__ partial, int64_t P, double N, float ssim_weight,
                                                                 float depth_weight, float* __restrict__ totals) {
    __shared__ double wreal[4][3];
    __shared__ long long wcount[4];
    double l1 = 0.0, ss = 0.0, dd = 0.0;
    long long cnt = 0;
    for (int64_t p = threadIdx.x; p < P; p += 256) {
        const float* row = partial + p * COLS;
        l1 += (double)row[0];
        ss += (double)row[1];
        dd += (double)row[2];
        cnt += (long long)__float_as_int(row[3]);
    }
    l1 = butterfly_sum(l1);
    ss = butterfly_sum(ss);
    dd = butterfly_sum(dd);
    cnt = butterfly_sum(cnt);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wreal[wave][0] = l1; wreal[wave][1] = ss; wreal[wave][2] = dd; wcount[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double L = four_waves(wreal[0][0], wreal[1][0], wreal[2][0], wreal[3][0]);
        const double S = four_waves(wreal[0][1], wreal[1][1], wreal[2][1], wreal[3][1]);
        const double D = four_waves(wreal[0][2], wreal[1][2], wreal[2][2], wreal[3][2]);
        const long long count = four_waves(wcount[0], wcount[1], wcount[2], wcount[3]);
        const long long seen = count < 1 ? 1 : count;
        const float l1_mean = (float)(L / N), s_mean = (float)(S / N), d_mean = (float)(D / (double)seen);
        totals[0] = add(add(mul(sub(1.0f, ssim_weight), l1_mean), mul(ssim_weight, sub(1.0f, s_mean))), mul(depth_weight, d_mean));
        totals[1] = l1_mean;
        totals[2] = s_mean;
        totals[3] = d_mean;
        totals[4] = (float)seen;
        totals[5] = __int_as_float((int)(count > 0x7fffffffLL ? 0x7fffffffLL : count));
        totals[6] = 0.0f;
        totals[7] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void gauss_loss_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ targets,
                                                              const float* __restrict__ maps, const float* __restrict__ depth,
                                                              const float* __restrict__ depth_targets, const float* __restrict__ totals,
                                                              const float* __restrict__ upstream, int TX, int NT, int H, int W, float count,
                                                              float ssim_weight, float depth_weight, float* __restrict__ d_rgb,
                                                              float* __restrict__ d_depth) {
    __shared__ float ms[MAPS][APRON * APRON];
    __shared__ float rows[MAPS][APRON * TILE];
    const TileId id = tile_id(blockIdx.x, TX, NT);
    const int64_t vc = id.group;
    const int ti = id.ti, tj = id.tj;
    const int64_t plane = (int64_t)H * W;
#pragma unroll
    for (int k = 0; k < MAPS; ++k) stage_apron(maps + (vc * MAPS + k) * plane, ti, tj, H, W, ms[k]);
    __syncthreads();
    for (int k = threadIdx.x; k < APRON * TILE; k += 256) {
        const int r = k >> 4, c = k & (TILE - 1);
        float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
#pragma unroll
        for (int q = 0; q < TAPS; ++q) {
            const float w = tap(q);
            g0 = add(g0, mul(w, ms[0][r * APRON + c + q]));
            g1 = add(g1, mul(w, ms[1][r * APRON + c + q]));
            g2 = add(g2, mul(w, ms[2][r * APRON + c + q]));
        }
        rows[0][k] = g0; rows[1][k] = g1; rows[2][k] = g2;
    }
    __syncthreads();
    const int col = threadIdx.x & (TILE - 1), row = threadIdx.x >> 4;
    const int i = ti * TILE + col, j = tj * TILE + row;
    if (!(i < W && j < H)) return;                                          // no barrier follows
    float gm[MAPS];
    window_vertical(rows, row, col, gm);
    const float g0 = gm[0], g1 = gm[1], g2 = gm[2];
    const int64_t pix = (int64_t)j * W + i;
    const float x = rgb[vc * plane + pix], y = targets[vc * plane + pix];
    const float up = upstream[0];
    const float g = add(add(g0, mul(mul(2.0f, x), g1)), mul(y, g2));
    const float kl = dvd(sub(1.0f, ssim_weight), count), ks = dvd(ssim_weight, count);
    d_rgb[vc * plane + pix] = mul(up, sub(mul(kl, sgn(sub(x, y))), mul(ks, g)));
    if (d_depth && vc % 3 == 0) {
        const int64_t o = (vc / 3) * plane + pix;
        const float want = depth_targets[o];
        const float kd = dvd(depth_weight, totals[4]);
        d_depth[o] = mul(up, mul(kd, want > 0.0f ? sgn(sub(depth[o], want)) : 0.0f));
    }
}

// the image, the tile grid (V NT < 2^31) and the launch grid of one workgroup per (view, channel, tile)
inline int check_image(const char* name, int V, int H, int W) {
    MUDG_REQUIRE(V > 0 && H > 0 && W > 0, "%s: %d views of %d x %d", name, V, H, W);
    if (const int e = check_views(name, 1, V, H, W)) return e;
    const int64_t NT = GaussGrid(H, W).NT;
    MUDG_REQUIRE(3 * (int64_t)V * NT <= 0x7fffffffLL, "%s: %d views of 3 x %lld tiles are more workgroups than a grid holds", name, V,
                 (long long)NT);
    return MUDG_OK;
}

inline int check_weights(const char* name, float ssim_weight, float depth_weight) {
    MUDG_REQUIRE(ssim_weight >= 0.0f && ssim_weight <= 1.0f, "%s: an SSIM weight of %g (0 .. 1)", name, (double)ssim_weight);
    MUDG_REQUIRE(std::isfinite(depth_weight) && depth_weight >= 0.0f, "%s: a depth weight of %g (finite, not negative)", name,
                 (double)depth_weight);
    return MUDG_OK;
}

}  // namespace

extern "C" int mudg_gauss_loss(const float* rgb, const float* targets, const float* depth, const float* depth_targets, int V, int H, int W,
                               float* maps, float* partial, void* stream) {
    MUDG_REQUIRE(rgb && targets && maps && partial, "mudg_gauss_loss: null argument");
    MUDG_REQUIRE((depth == nullptr) == (depth_targets == nullptr), "mudg_gauss_loss: depth and depth_targets come together or not at all");
    MUDG_REQUIRE(aligned4(rgb) && aligned4(targets) && aligned4(depth) && aligned4(depth_targets) && aligned4(maps) && aligned4(partial),
                 "mudg_gauss_loss: unaligned argument");
    if (const int e = check_image("mudg_gauss_loss", V, H, W)) return e;
    const GaussGrid grid(H, W);
    hipLaunchKernelGGL(gauss_loss_kernel, dim3((unsigned)(3 * (int64_t)V * grid.NT)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rgb, targets,
                       depth, depth_targets, grid.TX, grid.NT, H, W, maps, partial);
    return mudg_check_launch("mudg_gauss_loss");
}

extern "C" int mudg_gauss_loss_finish(const float* partial, int V, int H, int W, float ssim_weight, float depth_weight, float* totals,
                                      void* stream) {
    MUDG_REQUIRE(partial && totals, "mudg_gauss_loss_finish: null argument");
    MUDG_REQUIRE(aligned4(partial) && aligned4(totals), "mudg_gauss_loss_finish: unaligned argument");
    if (const int e = check_image("mudg_gauss_loss_finish", V, H, W)) return e;
    if (const int e = check_weights("mudg_gauss_loss_finish", ssim_weight, depth_weight)) return e;
    const int64_t NT = GaussGrid(H, W).NT;
    hipLaunchKernelGGL(gauss_loss_finish_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partial, 3 * (int64_t)V * NT,
                       3.0 * (double)V * (double)H * (double)W, ssim_weight, depth_weight, totals);
    return mudg_check_launch("mudg_gauss_loss_finish");
}

extern "C" int mudg_gauss_loss_bwd(const float* rgb, const float* targets, const float* maps, const float* depth, const float* depth_targets,
                                   const float* totals, const float* upstream, int V, int H, int W, float ssim_weight, float depth_weight,
                                   float* d_rgb, float* d_depth, void* stream) {
    MUDG_REQUIRE(rgb && targets && maps && totals && upstream && d_rgb, "mudg_gauss_loss_bwd: null argument");
    MUDG_REQUIRE((depth == nullptr) == (depth_targets == nullptr), "mudg_gauss_loss_bwd: depth and depth_targets come together or not at all");
    MUDG_REQUIRE(depth || !d_depth, "mudg_gauss_loss_bwd: d_depth without depth");
    MUDG_REQUIRE(aligned4(rgb) && aligned4(targets) && aligned4(maps) && aligned4(depth) && aligned4(depth_targets) && aligned4(totals) &&
                     aligned4(upstream) && aligned4(d_rgb) && aligned4(d_depth),
                 "mudg_gauss_loss_bwd: unaligned argument");
    if (const int e = check_image("mudg_gauss_loss_bwd", V, H, W)) return e;
    if (const int e = check_weights("mudg_gauss_loss_bwd", ssim_weight, depth_weight)) return e;
    const GaussGrid grid(H, W);
    const float count = (float)(3.0 * (double)V * (double)H * (double)W);   // N, rounded once
    hipLaunchKernelGGL(gauss_loss_bwd_kernel, dim3((unsigned)(3 * (int64_t)V * grid.NT)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rgb,
                       targets, maps, depth, depth_targets, totals, upstream, grid.TX, grid.NT, H, W, count, ssim_weight, depth_weight, d_rgb, d_depth);
    return mudg_check_launch("mudg_gauss_loss_bwd");
}
