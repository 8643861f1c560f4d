// consistency.hip — cross-view depth consistency of a set of views: which lifted pixels other views confirm.
//   view_flags        a lane owns four pixels of a row of one view (blockIdx.y): one byte per pixel, bit 0 usable (min_depth < z <
//                     max_depth and not sky — depth_unproject's validity), bit 1 dynamic (the label's bit of a 64-bit class mask)
//   view_consistency  a lane owns one pixel of the source view (blockIdx.y): its world point in fp64 as depth_unproject forms it, then
//                     for every witness of the view's list the projection into the witness, the (2r + 1)^2 pixels around the pixel that
//                     holds it, and one of three verdicts; per pixel the counts of "agree" and "violate" and the keep byte, per view six
//                     integer sums: wave shuffles, LDS across the waves, one set of 64-bit integer atomics per workgroup
// The source row, the witness ids and every witness's row are indexed by blockIdx.y and the loop counter alone: uniform addresses,
// scalar loads, a uniform trip count.  Every floating-point operation is a single correctly rounded fp64 one in a fixed order (no
// contraction) and every sum is an integer: no output depends on the order of execution, and all of them are bit-equal to the numpy
// definition in tests/consistency_reference.py.  A rule of this project's own: the reference merges clouds by concatenation.
#include "depth_shared.h"

namespace {

constexpr int TABLE_DOUBLES = 16;              // three rows of a rigid transform, fx, fy, cx, cy
constexpr int STATS = 6;                       // usable, tested, kept, sum agree, sum violate, pixels with a violation
constexpr int MAX_WITNESSES = 64;              // per view: the counts fit a byte, a workgroup's sums 32 bits
constexpr int MAX_RADIUS = 2;
constexpr double ZNEAR = 1e-4;                 // metres in front of a witness below which it gives no evidence
constexpr uint32_t USABLE = 1u, DYNAMIC = 2u;

__device__ __forceinline__ uint32_t flag_of(float z32, bool labelled, long long label, long long sky_label, unsigned long long dynamic_mask,
                                            double min_depth, double max_depth) {
    const double z = (double)z32;
    const bool sky = labelled && label == sky_label;
    const bool dynamic = labelled && label >= 0 && label < 64 && ((dynamic_mask >> label) & 1ull);
    return ((z > min_depth && z < max_depth && !sky) ? USABLE : 0u) | (dynamic ? DYNAMIC : 0u);      // not a number: not usable
}

template <int PX>
__global__ __launch_bounds__(256) void view_flags_kernel(const float* __restrict__ depth, const int64_t* __restrict__ labels, long long sky_label,
                                                          unsigned long long dynamic_mask, int hw, double min_depth, double max_depth,
                                                          uint8_t* __restrict__ flags) {
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;
    if (p >= hw) return;
    const int64_t at = (int64_t)blockIdx.y * hw + p;
    float z32[PX];
    long long label[PX];
    load_f32<PX>(depth + at, z32);
#pragma unroll
    for (int e = 0; e < PX; ++e) label[e] = 0;
    if (labels) {
        if (PX == 4) {
            const u32x4 a = ld16(labels + at), b = ld16(labels + at + 2);
            label[0] = (long long)(((unsigned long long)a.y << 32) | a.x); label[1] = (long long)(((unsigned long long)a.w << 32) | a.z);
            label[2] = (long long)(((unsigned long long)b.y << 32) | b.x); label[3] = (long long)(((unsigned long long)b.w << 32) | b.z);
        } else {
            label[0] = labels[at];
        }
    }
    uint32_t f[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) f[e] = flag_of(z32[e], labels != nullptr, label[e], sky_label, dynamic_mask, min_depth, max_depth);
    if (PX == 4) *reinterpret_cast<uint32_t*>(flags + at) = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
    else flags[at] = (uint8_t)f[0];
}

__device__ __forceinline__ unsigned wave_add(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// A workgroup covers 256 pixels of one view and a pixel has at most 64 verdicts: every workgroup sum is below 2^14.
__global__ __launch_bounds__(256) void view_consistency_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ flags,
                                                                const double* __restrict__ src_table, const double* __restrict__ wit_table,
                                                                const int* __restrict__ times, const int* __restrict__ witnesses, int V, int N,
                                                                int H, int W, int r, int min_agree, int max_violate, double rel_tol,
                                                                double abs_tol, uint8_t* __restrict__ agree, uint8_t* __restrict__ violate,
                                                                uint8_t* __restrict__ keep, unsigned long long* __restrict__ stats) {
    __shared__ unsigned part[4][STATS];
    const int s = blockIdx.y;
    const int hw = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool inside = p < hw;
    const int64_t at = (int64_t)s * hw + (inside ? p : 0);
    const uint32_t mine = inside ? (uint32_t)flags[at] : 0u;
    const bool usable = (mine & USABLE) != 0, dynamic = (mine & DYNAMIC) != 0;
    unsigned n_agree = 0, n_violate = 0;
    if (usable) {                                                            // a pixel that is not usable does no projection
        const double* t = src_table + (int64_t)s * TABLE_DOUBLES;
        const double fx = t[12], fy = t[13], cx = t[14], cy = t[15];
        const int j = p / W, i = p - j * W;
        const double z = (double)depth[at];
        const double xn = __ddiv_rn(__dsub_rn(__dadd_rn((double)i, 0.5), cx), fx);
        const double yn = __ddiv_rn(__dsub_rn(__dadd_rn((double)j, 0.5), cy), fy);
        const double xc = __dmul_rn(xn, z), yc = __dmul_rn(yn, z);
        const double X = row4(t, xc, yc, z), Y = row4(t + 4, xc, yc, z), Z = row4(t + 8, xc, yc, z);
        const int time_s = times[s];
        for (int n = 0; n < N; ++n) {
            const int w = witnesses[(int64_t)s * N + n];
            if (w < 0 || w >= V || w == s) continue;                         // empty, out of range (the host rejects it), the view itself
            const bool same_time = times[w] == time_s;
            if (dynamic && !same_time) continue;
            const double* m = wit_table + (int64_t)w * TABLE_DOUBLES;
            const double qx = row4(m, X, Y, Z), qy = row4(m + 4, X, Y, Z), qz = row4(m + 8, X, Y, Z);
            if (!(qz > ZNEAR)) continue;
            const double u = __dadd_rn(__dmul_rn(m[12], __ddiv_rn(qx, qz)), m[14]);
            const double v = __dadd_rn(__dmul_rn(m[13], __ddiv_rn(qy, qz)), m[15]);
            if (!(u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)) continue;      // on doubles: 1e300 and what is not a number fall out here
            const int iw = (int)u, jw = (int)v;                              // 0 <= iw < W, 0 <= jw < H
            const int j0 = max(jw - r, 0), j1 = min(jw + r, H - 1), i0 = max(iw - r, 0), i1 = min(iw + r, W - 1);
            const double tol = __dadd_rn(abs_tol, __dmul_rn(rel_tol, qz));
            const int64_t base = (int64_t)w * hw;
            unsigned counting = 0, through = 0;
            bool agrees = false;
            for (int jj = j0; jj <= j1; ++jj) {
                for (int ii = i0; ii <= i1; ++ii) {                          // every address is inside the witness's image
                    const int64_t q = base + jj * W + ii;
                    const uint32_t f = flags[q];
                    if (!(f & USABLE) || (!same_time && (f & DYNAMIC))) continue;
                    const double d = __dsub_rn(qz, (double)depth[q]);
                    counting += 1u;
                    agrees = agrees || fabs(d) <= tol;
                    through += d < -tol ? 1u : 0u;
                }
            }
            if (agrees) n_agree += 1u;
            else if (counting && through == counting) n_violate += 1u;
        }
    }
    const bool kept = usable && (int)n_agree >= min_agree && (int)n_violate <= max_violate;
    if (inside) {                                                            // a pixel that is not usable stores 0, 0, 0
        agree[at] = (uint8_t)n_agree;
        violate[at] = (uint8_t)n_violate;
        keep[at] = kept ? 1 : 0;
    }
    unsigned sums[STATS] = {usable ? 1u : 0u, (n_agree | n_violate) ? 1u : 0u, kept ? 1u : 0u, n_agree, n_violate, n_violate ? 1u : 0u};
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < STATS; ++k) {
        sums[k] = wave_add(sums[k]);
        if ((threadIdx.x & 63) == 0) part[wave][k] = sums[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < STATS; ++k) {
            const unsigned total = part[0][k] + part[1][k] + part[2][k] + part[3][k];
            if (total) atomicAdd(stats + (int64_t)s * STATS + k, (unsigned long long)total);     // a sum of zero issues no atomic
        }
    }
}

}  // namespace

extern "C" int mudg_view_flags(const float* depth, const int64_t* labels, int64_t sky_label, uint64_t dynamic_mask, int views, int H, int W,
                               double min_depth, double max_depth, uint8_t* flags, void* stream) {
    MUDG_REQUIRE(depth && flags, "mudg_view_flags: null argument");
    MUDG_REQUIRE(shape_ok(views, H, W), "mudg_view_flags: %d views of %d x %d (1 .. 65535 views, at most 2^24 pixels each)", views, H, W);
    const int hw = H * W;
    const bool wide = (W & 3) == 0 && aligned16(depth) && aligned16(labels) && aligned4(flags);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned long long mask = (unsigned long long)dynamic_mask;
    if (wide) hipLaunchKernelGGL(view_flags_kernel<4>, frame_grid(views, hw, 4), dim3(256), 0, s, depth, labels, (long long)sky_label, mask, hw, min_depth, max_depth, flags);
    else hipLaunchKernelGGL(view_flags_kernel<1>, frame_grid(views, hw, 1), dim3(256), 0, s, depth, labels, (long long)sky_label, mask, hw, min_depth, max_depth, flags);
    return mudg_check_launch("mudg_view_flags");
}

extern "C" int mudg_view_consistency(const float* depth, const uint8_t* flags, const double* src_table, const double* wit_table,
                                     const int32_t* times, const int32_t* witnesses, int views, int N, int H, int W, int r, int min_agree,
                                     int max_violate, double rel_tol, double abs_tol, uint8_t* agree, uint8_t* violate, uint8_t* keep,
                                     uint64_t* stats, void* stream) {
    MUDG_REQUIRE(depth && flags && src_table && wit_table && times && witnesses && agree && violate && keep && stats,
                 "mudg_view_consistency: null argument");
    MUDG_REQUIRE(shape_ok(views, H, W), "mudg_view_consistency: %d views of %d x %d (1 .. 65535 views, at most 2^24 pixels each)", views, H, W);
    MUDG_REQUIRE(N >= 1 && N <= MAX_WITNESSES, "mudg_view_consistency: %d witnesses per view (1 .. %d)", N, MAX_WITNESSES);
    MUDG_REQUIRE(r >= 0 && r <= MAX_RADIUS, "mudg_view_consistency: window radius %d (0 .. %d)", r, MAX_RADIUS);
    MUDG_REQUIRE(min_agree >= 0 && max_violate >= 0, "mudg_view_consistency: min_agree %d, max_violate %d (not negative)", min_agree, max_violate);
    MUDG_REQUIRE(rel_tol >= 0.0 && abs_tol >= 0.0, "mudg_view_consistency: tolerances %g (relative) and %g m (not negative, numbers)", rel_tol, abs_tol);
    hipLaunchKernelGGL(view_consistency_kernel, frame_grid(views, H * W, 1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth, flags,
                       src_table, wit_table, times, witnesses, views, N, H, W, r, min_agree, max_violate, rel_tol, abs_tol, agree, violate, keep,
                       reinterpret_cast<unsigned long long*>(stats));
    return mudg_check_launch("mudg_view_consistency");
}
