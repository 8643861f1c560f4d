// gaussians_density.hip — adaptive density control for the Gaussian fit: which Gaussians a fit clones, splits and prunes,
// and the pass that rewrites the parameters and their Adam moments accordingly.
//   gauss_density_accumulate  a lane owns a Gaussian: per view it sums columns 8 and 9 (du, dv) of the Gaussian's partials in ascending
//                             order, takes the norm of that gradient in [-1, 1] screen units and adds it to grad_sum; seen counts the views
//   gauss_density_plan        a lane owns a Gaussian: prune, split, clone or keep, and how many rows that leaves
//   gauss_density_apply       a lane owns a source Gaussian and writes its rows of the fifteen tensors (five parameters, two moments each)
//                             and of ids at start[g]; survivors keep their order, a Gaussian's children are adjacent
// Everything is fp32, each operation a single rounded one in the order DESIGN.md §25 writes it, so every output is bit-equal to the numpy
// definition in tests/gaussians_density_reference.py and a repeat run gives the same bits.  No atomics, no generator state, no
// transcendental: the caller evaluates exp(log_scale), the rotation and log(split_shrink).  No MFMA operand is touched.
#include "gauss_shared.h"

namespace {

constexpr int KEEP = 0, PRUNE = 1, CLONE = 2, SPLIT = 3;
constexpr int TENSORS = 15;                         // 3 p + k: parameter p (xyz, colour, log_scale, quat, opacity_logit), k = value, m, v
constexpr int P_XYZ = 0, P_LOG_SCALE = 2;

struct DensityRows {
    const float* src[TENSORS];
    float* dst[TENSORS];
};

__global__ __launch_bounds__(256) void gauss_density_accumulate_kernel(const float* __restrict__ partial, const int32_t* __restrict__ count,
                                                                        const int64_t* __restrict__ offsets, int64_t n, int V, float half_w,
                                                                        float half_h, int64_t E, float* __restrict__ grad_sum,
                                                                        int32_t* __restrict__ seen) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    float total = grad_sum[idx];
    int32_t views = seen[idx];
    for (int view = 0; view < V; ++view) {
        with_partials<SUM_U, 2>(partial, count, offsets, (int64_t)view * n + idx, E, [&](const float (&s)[2]) {         // du, dv
            const float a = mul(half_w, s[0]), b = mul(half_h, s[1]);
            total = add(total, sqrtf(add(mul(a, a), mul(b, b))));          // sqrtf: the correctly rounded root (__fsqrt_rn is the native one)
            views += 1;
        });
    }
    grad_sum[idx] = total;
    seen[idx] = views;
}

__global__ __launch_bounds__(256) void gauss_density_plan_kernel(const float* __restrict__ grad_sum, const int32_t* __restrict__ seen,
                                                                  const float* __restrict__ opacity, const float* __restrict__ scale, int64_t n,
                                                                  float grad_threshold, float split_scale, float min_opacity, float max_scale,
                                                                  int grow, int32_t* __restrict__ action, int32_t* __restrict__ rows) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float gs = grad_sum[idx], op = opacity[idx];
    const int32_t sn = seen[idx];
    const float s0 = scale[3 * idx], s1 = scale[3 * idx + 1], s2 = scale[3 * idx + 2];
    const float smax = fmaxf(fmaxf(s0, s1), s2);
    int act = KEEP;
    if (gs != gs || op != op || s0 != s0 || s1 != s1 || s2 != s2 || op < min_opacity || smax > max_scale) {
        act = PRUNE;
    } else if (grow && sn > 0 && dvd(gs, (float)sn) >= grad_threshold) {
        act = smax > split_scale ? SPLIT : CLONE;
    }
    action[idx] = act;
    rows[idx] = act == PRUNE ? 0 : (act == KEEP ? 1 : 2);
}

__global__ __launch_bounds__(256) void gauss_density_apply_kernel(const int32_t* __restrict__ action, const int64_t* __restrict__ start,
                                                                   int64_t n, int64_t n_out, const float* __restrict__ scale,
                                                                   const float* __restrict__ rot, float split_offset, float log_shrink,
                                                                   DensityRows t, const int32_t* __restrict__ ids,
                                                                   int32_t* __restrict__ ids_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int act = action[idx];
    if (act != KEEP && act != CLONE && act != SPLIT) return;                // a prune, and every code that is none of the four
    const int copies = act == KEEP ? 1 : 2;
    const int64_t at = start[idx];
    if (at < 0 || at > n_out - copies) return;                              // not this plan's rows
    float shift[4] = {0.0f, 0.0f, 0.0f, 0.0f};                             // (d axis, -): indexed by a column of any parameter
    if (act == SPLIT) {
        const float s0 = scale[3 * idx], s1 = scale[3 * idx + 1], s2 = scale[3 * idx + 2];
        const int k = (s0 >= s1 && s0 >= s2) ? 0 : (s1 >= s2 ? 1 : 2);     // the first index of the largest scale
        const float d = mul(split_offset, k == 0 ? s0 : (k == 1 ? s1 : s2));
#pragma unroll
        for (int r = 0; r < 3; ++r) shift[r] = mul(d, rot[9 * idx + 3 * r + k]);
    }
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        const int width = p == 3 ? 4 : (p == 4 ? 1 : 3);
#pragma unroll
        for (int c = 0; c < width; ++c) {
            const float x = t.src[3 * p][width * idx + c];
            const float m = t.src[3 * p + 1][width * idx + c], v = t.src[3 * p + 2][width * idx + c];
            for (int r = 0; r < copies; ++r) {
                float y = x;
                if (act == SPLIT && p == P_XYZ) y = r == 0 ? add(x, shift[c]) : sub(x, shift[c]);
                if (act == SPLIT && p == P_LOG_SCALE) y = sub(x, log_shrink);
                const bool carries = act == KEEP || (act == CLONE && r == 0);       // every other row starts its moments at zero
                const int64_t o = width * (at + r) + c;
                t.dst[3 * p][o] = y;
                t.dst[3 * p + 1][o] = carries ? m : 0.0f;
                t.dst[3 * p + 2][o] = carries ? v : 0.0f;
            }
        }
    }
    if (ids) {
        const int32_t id = ids[idx];
        for (int r = 0; r < copies; ++r) ids_out[at + r] = id;
    }
}

inline bool rows_ok(int64_t n) { return n >= 1 && n <= 0x7fffffffLL; }

}  // namespace

extern "C" int mudg_gauss_density_accumulate(const float* partial, const int32_t* count, const int64_t* offsets, int64_t n, int V, int H, int W,
                                             int64_t E, float* grad_sum, int32_t* seen, void* stream) {
    MUDG_REQUIRE(partial && count && offsets && grad_sum && seen, "mudg_gauss_density_accumulate: null argument");
    MUDG_REQUIRE(aligned8(offsets), "mudg_gauss_density_accumulate: unaligned offsets");
    if (const int e = check_views("mudg_gauss_density_accumulate", n, V, H, W)) return e;
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_density_accumulate: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_density_accumulate: %lld entries (1 .. 2^31 - 1)", (long long)E);
    hipLaunchKernelGGL(gauss_density_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       partial, count, offsets, n, V, 0.5f * (float)W, 0.5f * (float)H, E, grad_sum, seen);
    return mudg_check_launch("mudg_gauss_density_accumulate");
}

extern "C" int mudg_gauss_density_plan(const float* grad_sum, const int32_t* seen, const float* opacity, const float* scale, int64_t n,
                                       float grad_threshold, float split_scale, float min_opacity, float max_scale, int grow, int32_t* action,
                                       int32_t* rows, void* stream) {
    MUDG_REQUIRE(grad_sum && seen && opacity && scale && action && rows, "mudg_gauss_density_plan: null argument");
    MUDG_REQUIRE(rows_ok(n), "mudg_gauss_density_plan: %lld Gaussians (1 .. 2^31 - 1)", (long long)n);
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_density_plan: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    MUDG_REQUIRE(!std::isnan(grad_threshold) && !std::isnan(split_scale) && !std::isnan(min_opacity) && !std::isnan(max_scale),
                 "mudg_gauss_density_plan: thresholds %g %g %g %g are numbers", (double)grad_threshold, (double)split_scale, (double)min_opacity,
                 (double)max_scale);
    hipLaunchKernelGGL(gauss_density_plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), grad_sum,
                       seen, opacity, scale, n, grad_threshold, split_scale, min_opacity, max_scale, grow, action, rows);
    return mudg_check_launch("mudg_gauss_density_plan");
}

extern "C" int mudg_gauss_density_apply(const int32_t* action, const int64_t* start, int64_t n, int64_t n_out, const float* scale,
                                        const float* rot, float split_offset, float log_shrink, const float* const* src, float* const* dst,
                                        const int32_t* ids, int32_t* ids_out, void* stream) {
    MUDG_REQUIRE(action && start && scale && rot && src && dst, "mudg_gauss_density_apply: null argument");
    MUDG_REQUIRE((ids == nullptr) == (ids_out == nullptr), "mudg_gauss_density_apply: ids and ids_out come together or not at all");
    DensityRows t;
    for (int k = 0; k < TENSORS; ++k) {                                     // the two tables are host arrays, read before the call returns
        MUDG_REQUIRE(src[k] && dst[k], "mudg_gauss_density_apply: null argument (tensor %d of %d)", k, TENSORS);
        t.src[k] = src[k];
        t.dst[k] = dst[k];
    }
    MUDG_REQUIRE(aligned8(start), "mudg_gauss_density_apply: unaligned start");
    MUDG_REQUIRE(rows_ok(n), "mudg_gauss_density_apply: %lld Gaussians (1 .. 2^31 - 1)", (long long)n);
    MUDG_REQUIRE(rows_ok(n_out), "mudg_gauss_density_apply: %lld rows out (1 .. 2^31 - 1)", (long long)n_out);
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_density_apply: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    MUDG_REQUIRE(!std::isnan(split_offset) && !std::isnan(log_shrink), "mudg_gauss_density_apply: split offset %g and log shrink %g are numbers",
                 (double)split_offset, (double)log_shrink);
    hipLaunchKernelGGL(gauss_density_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), action,
                       start, n, n_out, scale, rot, split_offset, log_shrink, t, ids, ids_out);
    return mudg_check_launch("mudg_gauss_density_apply");
}
