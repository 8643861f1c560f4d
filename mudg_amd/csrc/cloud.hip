// cloud.hip — the scene's point clouds from LiDAR sweeps.
//   cloud_sweep          a lane owns one LiDAR return of one frame (blockIdx.y): to the world, coloured by the last camera that sees
//                        it, labelled by the first visible box that holds it; one 16-byte packed point and one int32 label per lane
//                                                                                  process_lidar.py:27-33, 45-82, 121-138, 229-250
//   cloud_voxel_keys     a lane owns a point: the 63-bit key of its voxel on an absolute grid
//   cloud_voxel_reduce   a lane owns a point of the key-sorted order: integer sums per voxel, reduced across the wave's runs of equal
//                        segment id with shuffles, one set of integer atomics per (wave, segment)
//   cloud_voxel_finish   a lane owns a voxel: the mean position and the round-half-up mean colour, packed
// The arithmetic is fp64 in a fixed order with correctly rounded operations (no contraction) and every sum is an integer: no output
// depends on the order of execution, and all of them are bit-equal to the numpy definition in tests/cloud_reference.py.
#include "common.h"

namespace {

constexpr int CAM_DOUBLES = 24;        // w2c[12], K[9], then three int64: h, w, byte offset of the image
constexpr int OBJ_DOUBLES = 16;        // w2l[12], box extents[3], visible (non-zero)
constexpr int MAX_CAMERAS = 8;
constexpr int SUMS = 8;                // per voxel: count, r, g, b, fx, fy, fz, key

// ((m0 x + m1 y) + m2 z) (+ m3)
__device__ __forceinline__ double row3(const double* m, double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z));
}
__device__ __forceinline__ double row4(const double* m, double x, double y, double z) { return __dadd_rn(row3(m, x, y, z), m[3]); }

// astype(int32) of a value that fits; a value that does not fit (or is not a number) is outside every image
__device__ __forceinline__ bool fits_int32(double v) { return v > -2147483649.0 && v < 2147483648.0; }

// The tables are indexed by blockIdx.y alone: uniform addresses, which the compiler keeps in scalar registers.
__global__ __launch_bounds__(256) void cloud_sweep_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                           const float* __restrict__ ranges, const int64_t* __restrict__ offsets,
                                                           int64_t total, const double* __restrict__ l2w, const double* __restrict__ cams,
                                                           int ncam, const double* __restrict__ objs, int nobj,
                                                           const uint8_t* __restrict__ images, int64_t image_bytes,
                                                           u32x4* __restrict__ points, int32_t* __restrict__ labels) {
    const int f = blockIdx.y;
    const int64_t first = offsets[f], count = offsets[f + 1] - first;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t idx = first + i;
    if (idx < 0 || idx >= total) return;                                    // an offset table that does not describe the buffers
    const float* o = rays_o + 3 * idx;
    const float* d = rays_d + 3 * idx;
    const double ox = (double)o[0], oy = (double)o[1], oz = (double)o[2];
    const double dx = (double)d[0], dy = (double)d[1], dz = (double)d[2];
    const double range = (double)ranges[idx];
    const double* m = l2w + (int64_t)f * 12;
    const double px = __dadd_rn(row4(m, ox, oy, oz), __dmul_rn(row3(m, dx, dy, dz), range));
    const double py = __dadd_rn(row4(m + 4, ox, oy, oz), __dmul_rn(row3(m + 4, dx, dy, dz), range));
    const double pz = __dadd_rn(row4(m + 8, ox, oy, oz), __dmul_rn(row3(m + 8, dx, dy, dz), range));

    bool seen = false;
    uint32_t colour = 0u;
    for (int c = 0; c < ncam; ++c) {
        const double* cam = cams + ((int64_t)f * ncam + c) * CAM_DOUBLES;
        const int64_t* dims = reinterpret_cast<const int64_t*>(cam + 21);
        const int64_t h = dims[0], w = dims[1], base = dims[2];
        const double zc = row4(cam + 8, px, py, pz);
        if (!(zc > 0.0)) continue;
        const double xn = __ddiv_rn(row4(cam, px, py, pz), zc), yn = __ddiv_rn(row4(cam + 4, px, py, pz), zc);
        const double x = __dadd_rn(__dadd_rn(__dmul_rn(cam[12], xn), __dmul_rn(cam[13], yn)), cam[14]);
        const double y = __dadd_rn(__dadd_rn(__dmul_rn(cam[15], xn), __dmul_rn(cam[16], yn)), cam[17]);
        if (!(fits_int32(x) && fits_int32(y))) continue;
        const int ix = (int)x, iy = (int)y;                                  // truncation toward zero: x in (-1, 0) is column 0
        if (!(ix >= 0 && ix < w && iy >= 0 && iy < h)) continue;
        const int64_t at = base + ((int64_t)iy * w + ix) * 3;               // the only data-dependent address, after the inside test
        if (at < 0 || at + 3 > image_bytes) continue;                        // a camera table that does not describe the image buffer
        colour = (uint32_t)images[at] | ((uint32_t)images[at + 1] << 8) | ((uint32_t)images[at + 2] << 16);
        seen = true;                                                         // the last camera that sees the point wins
    }

    int32_t label = seen ? 0 : -1;
    double x = px, y = py, z = pz;
    if (seen) {
        for (int k = 0; k < nobj; ++k) {
            const double* ob = objs + ((int64_t)f * nobj + k) * OBJ_DOUBLES;
            if (ob[15] == 0.0) continue;                                     // not visible in this frame (uniform)
            const double qx = row4(ob, px, py, pz), qy = row4(ob + 4, px, py, pz), qz = row4(ob + 8, px, py, pz);
            const double hx = __ddiv_rn(ob[12], 2.0), hy = __ddiv_rn(ob[13], 2.0), hz = __ddiv_rn(ob[14], 2.0);
            if (qx > -hx && qx < hx && qy > -hy && qy < hy && qz > __dadd_rn(-hz, 0.25) && qz < hz) {
                label = k + 1;                                               // the first box that holds the point
                x = qx; y = qy; z = qz;                                      // object points are kept in the object's frame
                break;
            }
        }
    }
    const u32x4 out = {__float_as_uint(__double2float_rn(x)), __float_as_uint(__double2float_rn(y)), __float_as_uint(__double2float_rn(z)), colour};
    points[idx] = out;
    labels[idx] = label;
}

// ---- voxel thinning ----------------------------------------------------------------------------------------------------------------
constexpr double TWO32 = 4294967296.0;

__device__ __forceinline__ long long voxel_index(float p, double v) { return (long long)floor(__ddiv_rn((double)p, v)); }

// floor((r / v) 2^32) clamped to [0, 2^32 - 1], r = p - i v
__device__ __forceinline__ unsigned long long voxel_offset(float p, long long i, double v) {
    const double r = __dsub_rn((double)p, __dmul_rn((double)i, v));
    double fr = floor(__dmul_rn(__ddiv_rn(r, v), TWO32));
    fr = fr >= 0.0 ? fr : 0.0;                                               // not a number: 0
    fr = fr <= 4294967295.0 ? fr : 4294967295.0;
    return (unsigned long long)fr;
}

__global__ __launch_bounds__(256) void cloud_voxel_keys_kernel(const u32x4* __restrict__ pts, int64_t n, double v, long long* __restrict__ keys) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const u32x4 q = pts[idx];
    const long long ix = voxel_index(__uint_as_float(q.x), v), iy = voxel_index(__uint_as_float(q.y), v), iz = voxel_index(__uint_as_float(q.z), v);
    keys[idx] = (long long)((((unsigned long long)(ix + (1 << 20)) & 0x1fffffull) << 42) | (((unsigned long long)(iy + (1 << 20)) & 0x1fffffull) << 21) |
                            ((unsigned long long)(iz + (1 << 20)) & 0x1fffffull));
}

template <typename T>
__device__ __forceinline__ void run_add(T& val, int o, bool take) {
    const T other = __shfl_down(val, o, 64);
    if (take) val += other;
}

// Lane j owns point order[j] of the key-sorted order; segments[j] is its voxel's rank.  Equal ranks are adjacent, so the lanes of a
// wave form runs: a segmented shuffle reduction leaves each run's sums in its first lane, which issues the atomics.
__global__ __launch_bounds__(256) void cloud_voxel_reduce_kernel(const u32x4* __restrict__ pts, const int64_t* __restrict__ order,
                                                                  const int64_t* __restrict__ segments, int64_t n, double v,
                                                                  unsigned long long* __restrict__ sums, int64_t voxels) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    long long seg = -1;                                                       // no lane beyond the cloud joins a run
    unsigned cnt = 0, r = 0, g = 0, b = 0;
    unsigned long long fx = 0, fy = 0, fz = 0, key = 0;
    if (j < n) {
        const int64_t src = order[j];
        const long long s = segments[j];
        if (src >= 0 && src < n && s >= 0 && s < voxels) {                    // an order or a ranking that is not this cloud's: dropped
            seg = s;
            const u32x4 q = pts[src];
            const float x = __uint_as_float(q.x), y = __uint_as_float(q.y), z = __uint_as_float(q.z);
            const long long ix = voxel_index(x, v), iy = voxel_index(y, v), iz = voxel_index(z, v);
            fx = voxel_offset(x, ix, v); fy = voxel_offset(y, iy, v); fz = voxel_offset(z, iz, v);
            cnt = 1; r = q.w & 0xffu; g = (q.w >> 8) & 0xffu; b = (q.w >> 16) & 0xffu;
            key = (((unsigned long long)(ix + (1 << 20)) & 0x1fffffull) << 42) | (((unsigned long long)(iy + (1 << 20)) & 0x1fffffull) << 21) |
                  ((unsigned long long)(iz + (1 << 20)) & 0x1fffffull);
        }
    }
    const long long before = __shfl_up(seg, 1, 64);
    const bool head = seg >= 0 && (lane == 0 || before != seg);
    // A run ends before the next head or dropped lane: a dropped entry inside a run of equal ranks splits it in two, each with a head of
    // its own, and neither takes the other's lanes (comparing ranks alone would add the second part twice).
    const unsigned long long ends = __ballot(head || seg < 0);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const bool take = seg >= 0 && lane + o < 64 && ((ends >> (lane + 1)) & ((1ull << o) - 1ull)) == 0ull;
        run_add(cnt, o, take); run_add(r, o, take); run_add(g, o, take); run_add(b, o, take);
        run_add(fx, o, take); run_add(fy, o, take); run_add(fz, o, take);
    }
    if (head) {
        unsigned long long* s = sums + seg * SUMS;
        atomicAdd(s + 0, (unsigned long long)cnt); atomicAdd(s + 1, (unsigned long long)r);
        atomicAdd(s + 2, (unsigned long long)g); atomicAdd(s + 3, (unsigned long long)b);
        atomicAdd(s + 4, fx); atomicAdd(s + 5, fy); atomicAdd(s + 6, fz);
        s[7] = key;                                                           // every writer of a voxel stores the same key
    }
}

__global__ __launch_bounds__(256) void cloud_voxel_finish_kernel(const unsigned long long* __restrict__ sums, int64_t voxels, double v,
                                                                  u32x4* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= voxels) return;
    const unsigned long long* s = sums + k * SUMS;
    const unsigned long long cnt = s[0], key = s[7];
    u32x4 q = {0u, 0u, 0u, 0u};
    if (cnt) {
        const double scale = __dmul_rn((double)cnt, TWO32);
        uint32_t w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const long long i = (long long)((key >> (42 - 21 * a)) & 0x1fffffull) - (1 << 20);
            const double mean = __dmul_rn(v, __ddiv_rn((double)s[4 + a], scale));
            w[a] = __float_as_uint(__double2float_rn(__dadd_rn(__dmul_rn((double)i, v), mean)));
        }
        const uint32_t r = (uint32_t)((2 * s[1] + cnt) / (2 * cnt)), g = (uint32_t)((2 * s[2] + cnt) / (2 * cnt)), b = (uint32_t)((2 * s[3] + cnt) / (2 * cnt));
        q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = r | (g << 8) | (b << 16);
    }
    out[k] = q;
}

inline bool grid_ok(int64_t lanes) { return (lanes + 255) / 256 <= 0x7fffffffLL; }

}  // namespace

extern "C" int mudg_cloud_sweep(const float* rays_o, const float* rays_d, const float* ranges, const int64_t* offsets, int frames,
                                int64_t max_rays, int64_t total, const double* l2w, const double* cams, int ncam, const double* objs,
                                int nobj, const uint8_t* images, int64_t image_bytes, void* points, int32_t* labels, void* stream) {
    MUDG_REQUIRE(rays_o && rays_d && ranges && offsets && l2w && points && labels, "mudg_cloud_sweep: bad arguments");
    MUDG_REQUIRE(frames > 0 && frames <= 65535 && max_rays > 0 && total > 0 && grid_ok(max_rays), "mudg_cloud_sweep: %d frames of up to %lld rays", frames, (long long)max_rays);
    MUDG_REQUIRE(ncam >= 0 && ncam <= MAX_CAMERAS && (ncam == 0 || (cams && images && image_bytes > 0)), "mudg_cloud_sweep: %d cameras (at most %d, with a table and images)", ncam, MAX_CAMERAS);
    MUDG_REQUIRE(nobj >= 0 && (nobj == 0 || objs), "mudg_cloud_sweep: %d objects without a table", nobj);
    MUDG_REQUIRE(aligned16(points), "mudg_cloud_sweep: unaligned points");
    const dim3 grid((unsigned)((max_rays + 255) / 256), (unsigned)frames);
    hipLaunchKernelGGL(cloud_sweep_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rays_o, rays_d, ranges, offsets, total, l2w,
                       cams, ncam, objs, nobj, images, image_bytes, reinterpret_cast<u32x4*>(points), labels);
    return mudg_check_launch("mudg_cloud_sweep");
}

extern "C" int mudg_cloud_voxel_keys(const void* points, int64_t n, double voxel, int64_t* keys, void* stream) {
    MUDG_REQUIRE(points && keys && n > 0 && grid_ok(n) && aligned16(points), "mudg_cloud_voxel_keys: bad arguments");
    MUDG_REQUIRE(voxel > 0.0 && voxel < 1e30, "mudg_cloud_voxel_keys: voxel size %g", voxel);
    hipLaunchKernelGGL(cloud_voxel_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(points), n, voxel, reinterpret_cast<long long*>(keys));
    return mudg_check_launch("mudg_cloud_voxel_keys");
}

extern "C" int mudg_cloud_voxel_reduce(const void* points, const int64_t* order, const int64_t* segments, int64_t n, double voxel,
                                       uint64_t* sums, int64_t voxels, void* stream) {
    MUDG_REQUIRE(points && order && segments && sums && n > 0 && voxels > 0 && voxels <= n && grid_ok(n) && aligned16(points), "mudg_cloud_voxel_reduce: bad arguments");
    MUDG_REQUIRE(voxel > 0.0 && voxel < 1e30, "mudg_cloud_voxel_reduce: voxel size %g", voxel);
    hipLaunchKernelGGL(cloud_voxel_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(points), order, segments, n, voxel, reinterpret_cast<unsigned long long*>(sums), voxels);
    return mudg_check_launch("mudg_cloud_voxel_reduce");
}

extern "C" int mudg_cloud_voxel_finish(const uint64_t* sums, int64_t voxels, double voxel, void* points_out, void* stream) {
    MUDG_REQUIRE(sums && points_out && voxels > 0 && grid_ok(voxels) && aligned16(points_out), "mudg_cloud_voxel_finish: bad arguments");
    MUDG_REQUIRE(voxel > 0.0 && voxel < 1e30, "mudg_cloud_voxel_finish: voxel size %g", voxel);
    hipLaunchKernelGGL(cloud_voxel_finish_kernel, dim3((unsigned)((voxels + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(sums), voxels, voxel, reinterpret_cast<u32x4*>(points_out));
    return mudg_check_launch("mudg_cloud_voxel_finish");
}
