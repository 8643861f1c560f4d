// neighbours.hip — fixed-radius neighbour search between packed clouds, and the sums a cloud-to-cloud score comes from.
//   cloud_neighbours<NEAREST>   a lane owns a query: its cell on the grid of edge c = r (1 + 2^-10), the nine key intervals (x + a, y + b,
//                               z - 1 .. z + 1) of the key-sorted reference by binary search, every candidate's squared distance in fp64;
//                               NEAREST: the smallest d2 <= r2 and the lowest original index that attains it; else min(count, cap)
//   metric_cloud                a lane owns eight d2 values: found, sum floor(sqrt(d2) 2^20), the counts of d2 <= t2[k]; wave shuffles,
//                               LDS across the waves, one set of 64-bit integer atomics per workgroup
// Every floating-point operation is a single correctly rounded fp64 one in a fixed order (no contraction); a minimum with a stated tie
// rule, a capped count and integer sums do not depend on the order of execution: all three are bit-equal to the numpy definition in
// tests/neighbours_reference.py.  There is no table to probe: every loop is a binary search over, or a walk inside, the key array.
// No MFMA operand is touched: the same code in every library build.
#include "common.h"

#include <cmath>

namespace {

constexpr long long HALF = 1 << 20;              // the key's field offset (§13)
constexpr long long CELL_MAX = HALF - 1;         // a neighbour cell beyond +-(2^20 - 1) holds nothing: reference cells end at 2^20 - 2
constexpr double QUERY_LIMIT = 1048577.0;        // a query with |q / c| >= 2^20 + 1 on some axis finds nothing
constexpr double MAX_RADIUS2 = 4096.0;           // r <= 64
constexpr double MAX_CELL = 64.0625;             // 64 (1 + 2^-10)
constexpr int MAX_THRESHOLDS = 8;
constexpr int PER_LANE = 8;                      // metric_cloud: values per lane
constexpr double D_SCALE = 1048576.0;            // distances are summed on a 2^-20 grid

__device__ __forceinline__ long long cell_key(long long ix, long long iy, long long iz) {
    return (long long)(((unsigned long long)(ix + HALF) << 42) | ((unsigned long long)(iy + HALF) << 21) | (unsigned long long)(iz + HALF));
}

// the first position in [lo, n) whose key is >= k (UPPER: > k); at most 64 halvings of n
template <bool UPPER>
__device__ __forceinline__ int64_t key_bound(const long long* __restrict__ keys, int64_t lo, int64_t n, long long k) {
    int64_t hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const long long v = keys[mid];
        if (UPPER ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Lane j owns query visit[j] (visit: a permutation of the queries in the order of their cells, so that a wave's lanes walk the same or
// adjacent intervals; NULL: j itself) and writes that query's slot.
template <bool NEAREST>
__global__ __launch_bounds__(256) void cloud_neighbours_kernel(const u32x4* __restrict__ ref, const long long* __restrict__ keys,
                                                                const int64_t* __restrict__ order, int64_t n,
                                                                const u32x4* __restrict__ queries, const int64_t* __restrict__ visit, int64_t nq,
                                                                double cell, double r2, int cap, double* __restrict__ d2_out,
                                                                int64_t* __restrict__ index_out, int32_t* __restrict__ count_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nq) return;
    const int64_t qi = visit ? visit[j] : j;
    if (qi < 0 || qi >= nq) return;                                           // a visiting order that is not these queries'
    const u32x4 q = queries[qi];
    const double qx = (double)__uint_as_float(q.x), qy = (double)__uint_as_float(q.y), qz = (double)__uint_as_float(q.z);
    const double tx = __ddiv_rn(qx, cell), ty = __ddiv_rn(qy, cell), tz = __ddiv_rn(qz, cell);

    double best = INFINITY;
    int64_t best_index = -1;
    int count = 0;
    if (fabs(tx) < QUERY_LIMIT && fabs(ty) < QUERY_LIMIT && fabs(tz) < QUERY_LIMIT) {   // false for a coordinate that is not finite
        const long long ix = (long long)floor(tx), iy = (long long)floor(ty), iz = (long long)floor(tz);
        const long long z0 = iz - 1 > -CELL_MAX ? iz - 1 : -CELL_MAX, z1 = iz + 1 < CELL_MAX ? iz + 1 : CELL_MAX;
        for (int a = -1; a <= 1 && z0 <= z1 && (NEAREST || count < cap); ++a) {
            const long long cx = ix + a;
            if (cx < -CELL_MAX || cx > CELL_MAX) continue;
            for (int b = -1; b <= 1; ++b) {
                const long long cy = iy + b;
                if (cy < -CELL_MAX || cy > CELL_MAX) continue;
                if (!NEAREST && count >= cap) break;
                const int64_t first = key_bound<false>(keys, 0, n, cell_key(cx, cy, z0));
                const int64_t last = key_bound<true>(keys, first, n, cell_key(cx, cy, z1));
                for (int64_t s = first; s < last; ++s) {
                    const u32x4 p = ref[s];
                    const double dx = __dsub_rn(qx, (double)__uint_as_float(p.x)), dy = __dsub_rn(qy, (double)__uint_as_float(p.y)),
                                 dz = __dsub_rn(qz, (double)__uint_as_float(p.z));
                    const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                    if (!(d2 <= r2)) continue;
                    if (NEAREST) {
                        if (d2 <= best) {                                     // the index is read only where it can decide
                            const int64_t at = order[s];
                            if (d2 < best || at < best_index) { best = d2; best_index = at; }
                        }
                    } else if (++count >= cap) {
                        break;
                    }
                }
            }
        }
    }
    if (NEAREST) { d2_out[qi] = best; index_out[qi] = best_index; }
    else count_out[qi] = count < cap ? count : cap;
}

template <typename T>
__device__ __forceinline__ T wave_add(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Thresholds { double t2[MAX_THRESHOLDS]; };

// A workgroup covers 2048 values: its counts fit 32 bits, its sum of distances (each at most 2^26) does not.
__global__ __launch_bounds__(256) void metric_cloud_kernel(const double* __restrict__ d2, int64_t n, Thresholds th, int K, double r2,
                                                            unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[4][2 + MAX_THRESHOLDS];
    unsigned found = 0, within[MAX_THRESHOLDS] = {};
    unsigned long long dist = 0;
    const int64_t base = (int64_t)blockIdx.x * (256 * PER_LANE) + threadIdx.x;
#pragma unroll
    for (int e = 0; e < PER_LANE; ++e) {
        const int64_t i = base + e * 256;
        if (i >= n) break;
        const double v = d2[i];
        if (!(fabs(v) < INFINITY)) continue;                                  // nothing within reach (or not a number): not found
        const double inside = fmin(fmax(v, 0.0), r2);                         // a nearest-neighbour d2 is in [0, r2] already: the sum's headroom
        found += 1u;
        dist += (unsigned long long)floor(__dmul_rn(__dsqrt_rn(inside), D_SCALE));
#pragma unroll
        for (int k = 0; k < MAX_THRESHOLDS; ++k) within[k] += (k < K && v <= th.t2[k]) ? 1u : 0u;
    }
    found = wave_add(found);
    dist = wave_add(dist);
#pragma unroll
    for (int k = 0; k < MAX_THRESHOLDS; ++k) within[k] = wave_add(within[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = found;
        part[wave][1] = dist;
#pragma unroll
        for (int k = 0; k < MAX_THRESHOLDS; ++k) part[wave][2 + k] = within[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 + K) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(sums + threadIdx.x, v);                             // a workgroup with nothing to add issues no atomic
    }
}

inline bool grid_ok(int64_t lanes) { return (lanes + 255) / 256 <= 0x7fffffffLL; }

int check_search(const char* name, const void* ref, const int64_t* keys, const int64_t* order, int64_t n, const void* queries, int64_t nq,
                 double cell, double r2) {
    MUDG_REQUIRE(ref && keys && order && queries, "%s: null argument", name);
    MUDG_REQUIRE(aligned16(ref) && aligned16(queries), "%s: unaligned points", name);
    MUDG_REQUIRE(n > 0 && nq > 0 && grid_ok(nq), "%s: %lld reference points, %lld queries", name, (long long)n, (long long)nq);
    MUDG_REQUIRE(r2 > 0.0 && r2 <= MAX_RADIUS2, "%s: squared radius %g (0 < r <= 64)", name, r2);
    MUDG_REQUIRE(cell <= MAX_CELL && cell * cell > r2, "%s: cell edge %g at squared radius %g (r < cell <= 64 (1 + 2^-10))", name, cell, r2);
    return MUDG_OK;
}

}  // namespace

extern "C" int mudg_cloud_nearest(const void* ref_sorted, const int64_t* keys, const int64_t* order, int64_t n, const void* queries,
                                  const int64_t* visit, int64_t nq, double cell, double r2, double* d2, int64_t* index, void* stream) {
    if (const int e = check_search("mudg_cloud_nearest", ref_sorted, keys, order, n, queries, nq, cell, r2)) return e;
    MUDG_REQUIRE(d2 && index, "mudg_cloud_nearest: null argument");
    hipLaunchKernelGGL(cloud_neighbours_kernel<true>, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(ref_sorted), reinterpret_cast<const long long*>(keys), order, n,
                       reinterpret_cast<const u32x4*>(queries), visit, nq, cell, r2, 1, d2, index, (int32_t*)nullptr);
    return mudg_check_launch("mudg_cloud_nearest");
}

extern "C" int mudg_cloud_count(const void* ref_sorted, const int64_t* keys, const int64_t* order, int64_t n, const void* queries,
                                const int64_t* visit, int64_t nq, double cell, double r2, int cap, int32_t* counts, void* stream) {
    if (const int e = check_search("mudg_cloud_count", ref_sorted, keys, order, n, queries, nq, cell, r2)) return e;
    MUDG_REQUIRE(counts, "mudg_cloud_count: null argument");
    MUDG_REQUIRE(cap >= 1, "mudg_cloud_count: cap %d (at least 1)", cap);
    hipLaunchKernelGGL(cloud_neighbours_kernel<false>, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4*>(ref_sorted), reinterpret_cast<const long long*>(keys), order, n,
                       reinterpret_cast<const u32x4*>(queries), visit, nq, cell, r2, cap, (double*)nullptr, (int64_t*)nullptr, counts);
    return mudg_check_launch("mudg_cloud_count");
}

extern "C" int mudg_metric_cloud(const double* d2, int64_t n, const double* t2_host, int K, double r2, int64_t* sums, void* stream) {
    MUDG_REQUIRE(d2 && sums && (K == 0 || t2_host), "mudg_metric_cloud: null argument");
    MUDG_REQUIRE(n > 0 && n < 0x80000000LL, "mudg_metric_cloud: %lld values (1 .. 2^31 - 1)", (long long)n);
    MUDG_REQUIRE(K >= 0 && K <= MAX_THRESHOLDS, "mudg_metric_cloud: %d thresholds (at most %d)", K, MAX_THRESHOLDS);
    MUDG_REQUIRE(r2 > 0.0 && r2 <= MAX_RADIUS2, "mudg_metric_cloud: squared radius %g (0 < r <= 64)", r2);
    Thresholds th = {};
    for (int k = 0; k < K; ++k) {
        MUDG_REQUIRE(t2_host[k] > 0.0 && t2_host[k] <= r2, "mudg_metric_cloud: squared threshold %g (0 < t2 <= r2 = %g)", t2_host[k], r2);
        th.t2[k] = t2_host[k];
    }
    const int64_t per_block = 256 * PER_LANE;
    hipLaunchKernelGGL(metric_cloud_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       d2, n, th, K, r2, reinterpret_cast<unsigned long long*>(sums));
    return mudg_check_launch("mudg_metric_cloud");
}
