// normals.hip — the fourth dense modality, surface normals: made from depth, resized into clips, scored.
//   depth_normals   a depth map (frames, H, W) fp32 metres with its intrinsics -> camera-space unit normals (frames, H, W, 3) fp32 and a
//                   validity byte: §14's unprojection without the pose, central or one-sided differences over usable neighbours, n = dy x dx
//   normal_stream   (T, H0, W0, 3) fp32 normal maps -> the three fp32 planes of a clip at any place of a (.., 3, T, H, W) tensor: §16's fp32
//                   linear rule per channel, nothing else                                            lvdm/data/waymo_data.py:194-265
//   metric_normals  a generated normal stream's bytes against true normals: per frame 720 integer counts of the angle between them in
//                   quarter-degree bins, the cosine compared with a table the host made — no kernel evaluates an inverse cosine
// Every floating-point operation is a single correctly rounded one in a stated order (no contraction) and every reduction is an integer
// one: no output depends on the order of execution, and all of them are bit-equal to the numpy definition in tests/normals_reference.py.
// depth_normals is shaped as depth.hip's kernels: blockIdx.y is the frame (the table's address is uniform: scalar loads), a lane owns four
// consecutive pixels of a row (PX = 4) or one (W % 4 != 0, unaligned bases); the rows above and below come straight from global memory.
// No MFMA operand is touched: the same code in every library build.
#include "depth_shared.h"
#include "frames_shared.h"

namespace {

constexpr int BINS = 720;                      // quarter degrees of [0, 180]
constexpr int STREAM_BLOCK = 128;              // normal_stream: lanes per workgroup, 512 output pixels of one row
constexpr int STREAM_PX = 4;
constexpr int SCORE_PIXELS = 8192;             // metric_normals: a workgroup takes at least this many pixels of a frame (if it has them)
constexpr int SCORE_GROUPS = 32;               // and a frame at most this many workgroups

__device__ __forceinline__ bool usable(double z, bool sky, double lo, double hi) { return z > lo && z < hi && !sky; }   // not a number: no

// a neighbour counts: it is usable and, under the step limit r >= 0, |z_nb - z| <= r z
__device__ __forceinline__ bool counts(double znb, bool ok, double z, double r) {
    return ok && (r < 0.0 || fabs(__dsub_rn(znb, z)) <= __dmul_rn(r, z));
}

// P(plus) - P(minus) for two points on the rays (xp, yp, 1) zp and (xm, ym, 1) zm
__device__ __forceinline__ void point_difference(double xp, double yp, double zp, double xm, double ym, double zm, double (&d)[3]) {
    d[0] = __dsub_rn(__dmul_rn(xp, zp), __dmul_rn(xm, zm));
    d[1] = __dsub_rn(__dmul_rn(yp, zp), __dmul_rn(ym, zm));
    d[2] = __dsub_rn(zp, zm);
}

template <int PX>
__global__ __launch_bounds__(256) void depth_normals_kernel(const float* __restrict__ depth, const int64_t* __restrict__ labels,
                                                             long long sky_label, const double* __restrict__ table, int H, int W,
                                                             double min_depth, double max_depth, double max_rel_step,
                                                             float* __restrict__ normals, uint8_t* __restrict__ valid) {
    const int f = blockIdx.y;
    const int hw = H * W;
    const int p = (blockIdx.x * 256 + threadIdx.x) * PX;                     // the lane's first pixel of the frame
    if (p >= hw) return;
    const double* t = table + (int64_t)f * 4;
    const double fx = t[0], fy = t[1], cx = t[2], cy = t[3];
    const int64_t base = (int64_t)f * hw;
    const float* d = depth + base;
    const int64_t* lab = labels ? labels + base : nullptr;
    const int j = p / W, i0 = p - j * W;                                     // PX = 4: W % 4 == 0, the four pixels share the row

    // depths and usability: the lane's pixels with the column before and after (c), the row above (u) and below (d); what is outside
    // the frame is not usable and is not read
    float z32[PX], zu32[PX], zd32[PX];
    bool sky[PX], skyu[PX], skyd[PX];
    double zc[PX + 2], zu[PX], zd[PX];
    bool okc[PX + 2], oku[PX], okd[PX];
    load_f32<PX>(d + p, z32);
    load_sky<PX>(lab, p, sky_label, sky);
#pragma unroll
    for (int e = 0; e < PX; ++e) { zc[e + 1] = (double)z32[e]; okc[e + 1] = usable(zc[e + 1], sky[e], min_depth, max_depth); }
    zc[0] = zc[PX + 1] = 0.0;
    okc[0] = okc[PX + 1] = false;
    if (i0 > 0) { zc[0] = (double)d[p - 1]; okc[0] = usable(zc[0], lab && lab[p - 1] == sky_label, min_depth, max_depth); }
    if (i0 + PX < W) { zc[PX + 1] = (double)d[p + PX]; okc[PX + 1] = usable(zc[PX + 1], lab && lab[p + PX] == sky_label, min_depth, max_depth); }
#pragma unroll
    for (int e = 0; e < PX; ++e) { zu[e] = zd[e] = 0.0; oku[e] = okd[e] = false; }
    if (j > 0) {
        load_f32<PX>(d + p - W, zu32);
        load_sky<PX>(lab, (int64_t)p - W, sky_label, skyu);
#pragma unroll
        for (int e = 0; e < PX; ++e) { zu[e] = (double)zu32[e]; oku[e] = usable(zu[e], skyu[e], min_depth, max_depth); }
    }
    if (j + 1 < H) {
        load_f32<PX>(d + p + W, zd32);
        load_sky<PX>(lab, (int64_t)p + W, sky_label, skyd);
#pragma unroll
        for (int e = 0; e < PX; ++e) { zd[e] = (double)zd32[e]; okd[e] = usable(zd[e], skyd[e], min_depth, max_depth); }
    }

    // the rays: xn of columns i0 - 1 .. i0 + PX, yn of rows j - 1 .. j + 1 (§14's expressions)
    double xn[PX + 2], yn[3];
#pragma unroll
    for (int e = 0; e < PX + 2; ++e) xn[e] = __ddiv_rn(__dsub_rn(__dadd_rn((double)(i0 - 1 + e), 0.5), cx), fx);
#pragma unroll
    for (int e = 0; e < 3; ++e) yn[e] = __ddiv_rn(__dsub_rn(__dadd_rn((double)(j - 1 + e), 0.5), cy), fy);

    float out[3 * PX];
    uint32_t good[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        const double z = zc[e + 1];
        const bool left = counts(zc[e], okc[e], z, max_rel_step), right = counts(zc[e + 2], okc[e + 2], z, max_rel_step);
        const bool up = counts(zu[e], oku[e], z, max_rel_step), down = counts(zd[e], okd[e], z, max_rel_step);
        double dx[3], dy[3];                                                 // a side that does not count is the centre itself
        point_difference(right ? xn[e + 2] : xn[e + 1], yn[1], right ? zc[e + 2] : z, left ? xn[e] : xn[e + 1], yn[1], left ? zc[e] : z, dx);
        point_difference(xn[e + 1], down ? yn[2] : yn[1], down ? zd[e] : z, xn[e + 1], up ? yn[0] : yn[1], up ? zu[e] : z, dy);
        const double nx = __dsub_rn(__dmul_rn(dy[1], dx[2]), __dmul_rn(dy[2], dx[1]));           // n = dy x dx
        const double ny = __dsub_rn(__dmul_rn(dy[2], dx[0]), __dmul_rn(dy[0], dx[2]));
        const double nz = __dsub_rn(__dmul_rn(dy[0], dx[1]), __dmul_rn(dy[1], dx[0]));
        const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(nx, nx), __dmul_rn(ny, ny)), __dmul_rn(nz, nz)));
        const bool ok = okc[e + 1] && (left || right) && (up || down) && len > 0.0 && len < __builtin_inf();
        good[e] = ok ? 1u : 0u;
        out[3 * e] = ok ? __double2float_rn(__ddiv_rn(nx, len)) : 0.0f;      // a pixel that is not valid stores zeros
        out[3 * e + 1] = ok ? __double2float_rn(__ddiv_rn(ny, len)) : 0.0f;
        out[3 * e + 2] = ok ? __double2float_rn(__ddiv_rn(nz, len)) : 0.0f;
    }
    float* dst = normals + (base + p) * 3;
    if (PX == 4) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const f32x4 o = {out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]};
            *reinterpret_cast<f32x4*>(dst + 4 * q) = o;
        }
        *reinterpret_cast<uint32_t*>(valid + base + p) = good[0] | (good[1] << 8) | (good[2] << 16) | (good[3] << 24);
    } else {
        dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
        valid[base + p] = (uint8_t)good[0];
    }
}

struct StreamArgs {
    const float* src;          // (T, H0, W0, 3) fp32
    const Tap* xt;             // W entries
    const Tap* yt;             // H entries
    float* dst;                // the first fp32 plane of the stream
    int H0, W0, H, W;
    int64_t cs, fs;            // channel and frame strides, in floats
};

// frames_kernel's fp32 branch with three interleaved source channels: blockIdx = (row segment, output row, frame)
template <bool WIDE>
__global__ __launch_bounds__(STREAM_BLOCK) void normal_stream_kernel(const StreamArgs a) {
    constexpr int PX = STREAM_PX;
    const int x0 = (blockIdx.x * STREAM_BLOCK + threadIdx.x) * PX;
    if (x0 >= a.W) return;
    const int y = blockIdx.y;
    const int64_t t = blockIdx.z;
    Tap ty = a.yt[y];
    ty.s0 = inside(ty.s0, a.H0); ty.s1 = inside(ty.s1, a.H0);
    const int n = WIDE ? PX : min(PX, a.W - x0);                              // WIDE: W % 4 == 0, all four exist
    const float* src = a.src + t * a.H0 * a.W0 * 3;
    const float* row0 = src + (int64_t)ty.s0 * a.W0 * 3;
    const float* row1 = src + (int64_t)ty.s1 * a.W0 * 3;
    float v[3][PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        Tap tx = a.xt[min(x0 + e, a.W - 1)];
        tx.s0 = inside(tx.s0, a.W0); tx.s1 = inside(tx.s1, a.W0);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            v[c][e] = linear_f32(row0[3 * tx.s0 + c], row0[3 * tx.s1 + c], row1[3 * tx.s0 + c], row1[3 * tx.s1 + c], tx, ty);
    }
    float* dst = a.dst + t * a.fs + (int64_t)y * a.W + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = dst + c * a.cs;
        if (WIDE) {
            const f32x4 o = {v[c][0], v[c][1], v[c][2], v[c][3]};
            *reinterpret_cast<f32x4*>(d) = o;
        } else {
#pragma unroll
            for (int e = 0; e < PX; ++e)
                if (e < n) d[e] = v[c][e];
        }
    }
}

// A workgroup walks its share of a frame, counts in LDS (32 bits hold a whole frame: at most 2^24 pixels) and adds its nonzero bins to
// the frame's 64-bit counts.  cosines: 721 doubles, descending from 1 to -1.
template <int PX>
__global__ __launch_bounds__(256) void metric_normals_kernel(const uint8_t* __restrict__ pred, const float* __restrict__ gt,
                                                              const uint8_t* __restrict__ valid, const double* __restrict__ cosines, int hw,
                                                              unsigned long long* __restrict__ hist) {
    __shared__ double edge[BINS + 1];
    __shared__ unsigned bin[BINS];
    for (int k = threadIdx.x; k <= BINS; k += 256) edge[k] = cosines[k];
    for (int k = threadIdx.x; k < BINS; k += 256) bin[k] = 0u;
    __syncthreads();
    const int f = blockIdx.y;
    const int64_t base = (int64_t)f * hw;
    for (int p = (blockIdx.x * 256 + threadIdx.x) * PX; p < hw; p += gridDim.x * 256 * PX) {
        const int64_t at = base + p;
        uint32_t u[3 * PX], use[PX];
        float g[3 * PX];
        if (PX == 4) {
            const u32x3 w = *reinterpret_cast<const u32x3*>(pred + at * 3);
            const uint32_t b[12] = {w.x & 255u, (w.x >> 8) & 255u, (w.x >> 16) & 255u, w.x >> 24, w.y & 255u, (w.y >> 8) & 255u,
                                    (w.y >> 16) & 255u, w.y >> 24, w.z & 255u, (w.z >> 8) & 255u, (w.z >> 16) & 255u, w.z >> 24};
#pragma unroll
            for (int e = 0; e < 12; ++e) u[e] = b[e];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(gt + at * 3 + 4 * q);
                g[4 * q] = v[0]; g[4 * q + 1] = v[1]; g[4 * q + 2] = v[2]; g[4 * q + 3] = v[3];
            }
            const uint32_t m = valid ? *reinterpret_cast<const uint32_t*>(valid + at) : 0xffffffffu;
            use[0] = m & 255u; use[1] = (m >> 8) & 255u; use[2] = (m >> 16) & 255u; use[3] = m >> 24;
        } else {
            u[0] = pred[at * 3]; u[1] = pred[at * 3 + 1]; u[2] = pred[at * 3 + 2];
            g[0] = gt[at * 3]; g[1] = gt[at * 3 + 1]; g[2] = gt[at * 3 + 2];
            use[0] = valid ? valid[at] : 1u;
        }
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            const int p0 = 2 * (int)u[3 * e] - 255, p1 = 2 * (int)u[3 * e + 1] - 255, p2 = 2 * (int)u[3 * e + 2] - 255;   // odd: never zero
            const double g0 = (double)g[3 * e], g1 = (double)g[3 * e + 1], g2 = (double)g[3 * e + 2];
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)p0, g0), __dmul_rn((double)p1, g1)), __dmul_rn((double)p2, g2));
            const double gg = __dadd_rn(__dadd_rn(__dmul_rn(g0, g0), __dmul_rn(g1, g1)), __dmul_rn(g2, g2));
            double c = __ddiv_rn(dot, __dsqrt_rn(__dmul_rn((double)(p0 * p0 + p1 * p1 + p2 * p2), gg)));
            if (!(use[e] && gg > 0.0 && gg < __builtin_inf() && c == c)) continue;
            c = fmin(fmax(c, -1.0), 1.0);
            int lo = 0, hi = BINS;                                           // the largest k with edge[k] >= c; edge[0] = 1 >= c
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (edge[mid] >= c) lo = mid; else hi = mid - 1;
            }
            atomicAdd(&bin[min(lo, BINS - 1)], 1u);                          // c = -1 = edge[720] belongs to the last bin
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < BINS; k += 256) {
        const unsigned n = bin[k];
        if (n) atomicAdd(hist + (int64_t)f * BINS + k, (unsigned long long)n);
    }
}

}  // namespace

extern "C" int mudg_depth_normals(const float* depth, const int64_t* labels, int64_t sky_label, const double* table, int frames, int H, int W,
                                  double min_depth, double max_depth, double max_rel_step, float* normals, uint8_t* valid, void* stream) {
    MUDG_REQUIRE(depth && table && normals && valid, "mudg_depth_normals: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_depth_normals: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    MUDG_REQUIRE(min_depth >= 0.0 && min_depth < max_depth, "mudg_depth_normals: depth range (%g, %g), expected 0 <= min_depth < max_depth", min_depth, max_depth);
    MUDG_REQUIRE(max_rel_step == max_rel_step, "mudg_depth_normals: the step limit is a number (negative: no limit)");
    const bool wide = (W & 3) == 0 && aligned16(depth) && aligned16(labels) && aligned16(normals) && aligned4(valid);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL(depth_normals_kernel<4>, frame_grid(frames, H * W, 4), dim3(256), 0, s, depth, labels, (long long)sky_label, table, H, W, min_depth, max_depth, max_rel_step, normals, valid);
    else hipLaunchKernelGGL(depth_normals_kernel<1>, frame_grid(frames, H * W, 1), dim3(256), 0, s, depth, labels, (long long)sky_label, table, H, W, min_depth, max_depth, max_rel_step, normals, valid);
    return mudg_check_launch("mudg_depth_normals");
}

extern "C" int mudg_normal_stream(const float* src, int T, int H0, int W0, int H, int W, const int32_t* xtab, const int32_t* ytab, float* dst,
                                  int64_t stream_stride, int64_t channel_stride, int64_t frame_stride, int slab, int frame0, void* stream) {
    MUDG_REQUIRE(src && dst && xtab && ytab, "mudg_normal_stream: null pointer");
    FRAMES_REQUIRE_SIZES("mudg_normal_stream");
    MUDG_REQUIRE(aligned16(xtab) && aligned16(ytab), "mudg_normal_stream: the tables are 16-byte entries, 16-byte aligned");
    MUDG_REQUIRE(frame_stride >= (int64_t)H * W && channel_stride > 0 && stream_stride >= 0 && slab >= 0 && frame0 >= 0,
                 "mudg_normal_stream: strides %lld / %lld / %lld at stream %d, frame %d (frames at least H W = %lld floats apart)",
                 (long long)stream_stride, (long long)channel_stride, (long long)frame_stride, slab, frame0, (long long)H * W);
    MUDG_REQUIRE(aligned4(src) && aligned4(dst), "mudg_normal_stream: the source and the destination are fp32");
    StreamArgs a = {};
    a.src = src; a.xt = reinterpret_cast<const Tap*>(xtab); a.yt = reinterpret_cast<const Tap*>(ytab);
    a.dst = dst + slab * stream_stride + frame0 * frame_stride;
    a.H0 = H0; a.W0 = W0; a.H = H; a.W = W; a.cs = channel_stride; a.fs = frame_stride;
    const bool wide = (W & 3) == 0 && aligned16(a.dst) && (channel_stride & 3) == 0 && (frame_stride & 3) == 0;
    const dim3 grid((unsigned)((W + STREAM_BLOCK * STREAM_PX - 1) / (STREAM_BLOCK * STREAM_PX)), (unsigned)H, (unsigned)T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL(normal_stream_kernel<true>, grid, dim3(STREAM_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(normal_stream_kernel<false>, grid, dim3(STREAM_BLOCK), 0, s, a);
    return mudg_check_launch("mudg_normal_stream");
}

extern "C" int mudg_metric_normals(const uint8_t* pred_u8, const float* gt, const uint8_t* valid, const double* cosines, int frames, int H, int W,
                                   int64_t* hist, void* stream) {
    MUDG_REQUIRE(pred_u8 && gt && cosines && hist, "mudg_metric_normals: null argument");
    MUDG_REQUIRE(shape_ok(frames, H, W), "mudg_metric_normals: %d frames of %d x %d (1 .. 65535 frames, at most 2^24 pixels each)", frames, H, W);
    const int hw = H * W;
    const bool wide = (hw & 3) == 0 && aligned4(pred_u8) && aligned16(gt) && aligned4(valid);
    const int share = (hw + SCORE_PIXELS - 1) / SCORE_PIXELS;                // hw >= 1: at least one workgroup
    const int groups = share < SCORE_GROUPS ? share : SCORE_GROUPS;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(hist);
    if (wide) hipLaunchKernelGGL(metric_normals_kernel<4>, dim3((unsigned)groups, (unsigned)frames), dim3(256), 0, s, pred_u8, gt, valid, cosines, hw, out);
    else hipLaunchKernelGGL(metric_normals_kernel<1>, dim3((unsigned)groups, (unsigned)frames), dim3(256), 0, s, pred_u8, gt, valid, cosines, hw, out);
    return mudg_check_launch("mudg_metric_normals");
}
