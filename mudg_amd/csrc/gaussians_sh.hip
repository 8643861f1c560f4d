// gaussians_sh.hip — view-dependent colour for the Gaussian splat renderer: real spherical harmonics of degrees 1 .. 3.
//   gauss_sh_colour  a lane owns a (view, Gaussian): the direction from the view's camera centre to the Gaussian in the Gaussian's own
//                    frame, the basis at that direction, colour + sum B_k sh[k - 1] clamped at zero; one colour per (view, Gaussian)
//   gauss_sh_bwd     a lane owns a Gaussian and walks the views in order: the colour columns of the blend's partials (§24) summed as
//                    gauss_project_bwd sums them, the forward recomputed bit for bit, and the gradients of colour, of the coefficients and,
//                    through the normalisation of the direction, of the position.  Plain stores, no atomics
//   gauss_sh_pose_bwd  a lane owns a (view, Gaussian): the same view's backward (sh_view_bwd, written once for both kernels), and what the
//                    position's share says about the view's matrix through c = -R^T t; summed over the Gaussians as DESIGN.md §28 orders it
// A workgroup's 256 coefficient rows are one contiguous piece of the (n, K - 1, 3) tensor.  It is fetched in whole 16-byte pieces, lane
// after lane, and handed out through LDS with an odd row stride (a lane's row then starts on its own bank); the backward's d_sh leaves
// the same way.  Everything is fp32, each operation a single rounded one in the order DESIGN.md §27 writes it, so both kernels are
// bit-equal to the numpy definition in tests/gaussians_sh_reference.py and a repeat run gives the same bits.
#include "gauss_shared.h"

namespace {

// the constants of the 3DGS code's real spherical harmonics, rounded once to fp32 (degree 0 is folded into `colour`)
constexpr float SH_C1 = 0.4886025119029199f;
constexpr float SH_C20 = 1.0925484305920792f, SH_C21 = -1.0925484305920792f, SH_C22 = 0.31539156525252005f, SH_C23 = -1.0925484305920792f,
                SH_C24 = 0.5462742152960396f;
constexpr float SH_C30 = -0.5900435899266435f, SH_C31 = 2.890611442640554f, SH_C32 = -0.4570457994644658f, SH_C33 = 0.3731763325901154f,
                SH_C34 = -0.4570457994644658f, SH_C35 = 1.445305721320277f, SH_C36 = -0.5900435899266435f;

template <int L>
struct ShShape {
    static constexpr int K = (L + 1) * (L + 1);     // basis functions, the constant one included
    static constexpr int ROW = 3 * (K - 1);         // floats of a Gaussian's coefficients: 9, 24, 45
    static constexpr int PAD = ROW | 1;             // the row's stride in LDS: odd, so 32 consecutive lanes read 32 banks
};

// ------------------------------------------------------------------------------------------------ a workgroup's rows through LDS
// Rows [256 b, min(n, 256 b + 256)) of an (n, ROW) tensor are floats [256 b ROW, ...): a 16-byte aligned start (the entry points check
// the tensor's), whole 16-byte pieces and at most three single floats at the cloud's end.
template <int L>
__device__ __forceinline__ int block_floats(int64_t n) {
    const int64_t left = n - (int64_t)blockIdx.x * 256;
    return (int)(left < 256 ? left : 256) * ShShape<L>::ROW;
}

template <int L>
__device__ __forceinline__ int lds_at(int f) {
    return ShShape<L>::PAD == ShShape<L>::ROW ? f : (f / ShShape<L>::ROW) * ShShape<L>::PAD + f % ShShape<L>::ROW;
}

// Ends with the barrier after which every lane may read its row at rows + threadIdx.x PAD.
template <int L>
__device__ __forceinline__ void stage_rows(const float* __restrict__ sh, int64_t n, float* rows) {
    const float* src = sh + (int64_t)blockIdx.x * 256 * ShShape<L>::ROW;
    const int total = block_floats<L>(n), pieces = total >> 2;
    for (int p = threadIdx.x; p < pieces; p += 256) {
        const f32x4 q = reinterpret_cast<const f32x4*>(src)[p];
        if constexpr (ShShape<L>::PAD == ShShape<L>::ROW) {
            reinterpret_cast<f32x4*>(rows)[p] = q;
        } else {
            rows[lds_at<L>(4 * p)] = q.x; rows[lds_at<L>(4 * p + 1)] = q.y; rows[lds_at<L>(4 * p + 2)] = q.z; rows[lds_at<L>(4 * p + 3)] = q.w;
        }
    }
    for (int f = 4 * pieces + threadIdx.x; f < total; f += 256) rows[lds_at<L>(f)] = src[f];
    __syncthreads();
}

// The way back: begins with the barrier after which every lane's row is in LDS.
template <int L>
__device__ __forceinline__ void store_rows(const float* rows, int64_t n, float* __restrict__ out) {
    __syncthreads();
    float* dst = out + (int64_t)blockIdx.x * 256 * ShShape<L>::ROW;
    const int total = block_floats<L>(n), pieces = total >> 2;
    for (int p = threadIdx.x; p < pieces; p += 256) {
        f32x4 q;
        if constexpr (ShShape<L>::PAD == ShShape<L>::ROW) {
            q = reinterpret_cast<const f32x4*>(rows)[p];
        } else {
            q.x = rows[lds_at<L>(4 * p)]; q.y = rows[lds_at<L>(4 * p + 1)]; q.z = rows[lds_at<L>(4 * p + 2)]; q.w = rows[lds_at<L>(4 * p + 3)];
        }
        reinterpret_cast<f32x4*>(dst)[p] = q;
    }
    for (int f = 4 * pieces + threadIdx.x; f < total; f += 256) dst[f] = rows[lds_at<L>(f)];
}

// ------------------------------------------------------------------------------------------------ the rule (§27)
struct ShPoint {
    float x, y, z;
    int id;
};

__device__ __forceinline__ ShPoint sh_point(const u32x4* __restrict__ pts, const int32_t* __restrict__ ids, int nmat, int64_t idx) {
    const u32x4 q = pts[idx];
    ShPoint p = {__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), 0};
    if (ids) { p.id = ids[idx]; p.id = p.id < 0 ? 0 : (p.id >= nmat ? nmat - 1 : p.id); }
    return p;
}

// d = (p - c) / |p - c| with c = -R^T t the camera centre in the Gaussian's own frame; len = |p - c|.
struct ShDir {
    float x, y, z, len;
};

__device__ __forceinline__ ShDir sh_direction(const float* __restrict__ m, const ShPoint& p) {
    const float cx = -add(add(mul(m[0], m[3]), mul(m[4], m[7])), mul(m[8], m[11]));
    const float cy = -add(add(mul(m[1], m[3]), mul(m[5], m[7])), mul(m[9], m[11]));
    const float cz = -add(add(mul(m[2], m[3]), mul(m[6], m[7])), mul(m[10], m[11]));
    const float vx = sub(p.x, cx), vy = sub(p.y, cy), vz = sub(p.z, cz);
    ShDir d;
    d.len = sqrtf(add(add(mul(vx, vx), mul(vy, vy)), mul(vz, vz)));        // sqrtf: the correctly rounded root (__fsqrt_rn is the native one)
    d.x = dvd(vx, d.len); d.y = dvd(vy, d.len); d.z = dvd(vz, d.len);
    return d;
}

// the products of the direction's components that degrees 2 and 3 share
struct ShPairs {
    float xx, yy, zz, xy, yz, xz;
    __device__ __forceinline__ explicit ShPairs(const ShDir& d)
        : xx(mul(d.x, d.x)), yy(mul(d.y, d.y)), zz(mul(d.z, d.z)), xy(mul(d.x, d.y)), yz(mul(d.y, d.z)), xz(mul(d.x, d.z)) {}
};

// B[1 .. K - 1]; B[0] is not used
template <int L>
__device__ __forceinline__ void sh_basis(const ShDir& d, float (&B)[ShShape<L>::K]) {
    const ShPairs q(d);
    B[0] = 0.0f;
    B[1] = mul(-SH_C1, d.y);
    B[2] = mul(SH_C1, d.z);
    B[3] = mul(-SH_C1, d.x);
    if constexpr (L >= 2) {
        B[4] = mul(SH_C20, q.xy);
        B[5] = mul(SH_C21, q.yz);
        B[6] = mul(SH_C22, sub(sub(mul(2.0f, q.zz), q.xx), q.yy));
        B[7] = mul(SH_C23, q.xz);
        B[8] = mul(SH_C24, sub(q.xx, q.yy));
    }
    if constexpr (L >= 3) {
        B[9] = mul(mul(SH_C30, d.y), sub(mul(3.0f, q.xx), q.yy));
        B[10] = mul(mul(SH_C31, q.xy), d.z);
        B[11] = mul(mul(SH_C32, d.y), sub(sub(mul(4.0f, q.zz), q.xx), q.yy));
        B[12] = mul(mul(SH_C33, d.z), sub(sub(mul(2.0f, q.zz), mul(3.0f, q.xx)), mul(3.0f, q.yy)));
        B[13] = mul(mul(SH_C34, d.x), sub(sub(mul(4.0f, q.zz), q.xx), q.yy));
        B[14] = mul(mul(SH_C35, d.z), sub(q.xx, q.yy));
        B[15] = mul(mul(SH_C36, d.x), sub(q.xx, mul(3.0f, q.yy)));
    }
}

// g = sum_k s[k] dB_k/dd, the terms in ascending k and within a k in the order x, y, z; every term is (constant polynomial) s[k]
template <int L>
__device__ __forceinline__ void sh_basis_grad(const ShDir& d, const float (&s)[ShShape<L>::K], float& gx, float& gy, float& gz) {
    const ShPairs q(d);
    gy = mul(-SH_C1, s[1]);
    gz = mul(SH_C1, s[2]);
    gx = mul(-SH_C1, s[3]);
    if constexpr (L >= 2) {
        gx = add(gx, mul(mul(SH_C20, d.y), s[4]));
        gy = add(gy, mul(mul(SH_C20, d.x), s[4]));
        gy = add(gy, mul(mul(SH_C21, d.z), s[5]));
        gz = add(gz, mul(mul(SH_C21, d.y), s[5]));
        gx = add(gx, mul(mul(SH_C22, mul(-2.0f, d.x)), s[6]));
        gy = add(gy, mul(mul(SH_C22, mul(-2.0f, d.y)), s[6]));
        gz = add(gz, mul(mul(SH_C22, mul(4.0f, d.z)), s[6]));
        gx = add(gx, mul(mul(SH_C23, d.z), s[7]));
        gz = add(gz, mul(mul(SH_C23, d.x), s[7]));
        gx = add(gx, mul(mul(SH_C24, mul(2.0f, d.x)), s[8]));
        gy = add(gy, mul(mul(SH_C24, mul(-2.0f, d.y)), s[8]));
    }
    if constexpr (L >= 3) {
        gx = add(gx, mul(mul(SH_C30, mul(6.0f, q.xy)), s[9]));
        gy = add(gy, mul(mul(SH_C30, sub(mul(3.0f, q.xx), mul(3.0f, q.yy))), s[9]));
        gx = add(gx, mul(mul(SH_C31, q.yz), s[10]));
        gy = add(gy, mul(mul(SH_C31, q.xz), s[10]));
        gz = add(gz, mul(mul(SH_C31, q.xy), s[10]));
        gx = add(gx, mul(mul(SH_C32, mul(-2.0f, q.xy)), s[11]));
        gy = add(gy, mul(mul(SH_C32, sub(sub(mul(4.0f, q.zz), q.xx), mul(3.0f, q.yy))), s[11]));
        gz = add(gz, mul(mul(SH_C32, mul(8.0f, q.yz)), s[11]));
        gx = add(gx, mul(mul(SH_C33, mul(-6.0f, q.xz)), s[12]));
        gy = add(gy, mul(mul(SH_C33, mul(-6.0f, q.yz)), s[12]));
        gz = add(gz, mul(mul(SH_C33, sub(sub(mul(6.0f, q.zz), mul(3.0f, q.xx)), mul(3.0f, q.yy))), s[12]));
        gx = add(gx, mul(mul(SH_C34, sub(sub(mul(4.0f, q.zz), mul(3.0f, q.xx)), q.yy)), s[13]));
        gy = add(gy, mul(mul(SH_C34, mul(-2.0f, q.xy)), s[13]));
        gz = add(gz, mul(mul(SH_C34, mul(8.0f, q.xz)), s[13]));
        gx = add(gx, mul(mul(SH_C35, mul(2.0f, q.xz)), s[14]));
        gy = add(gy, mul(mul(SH_C35, mul(-2.0f, q.yz)), s[14]));
        gz = add(gz, mul(mul(SH_C35, sub(q.xx, q.yy)), s[14]));
        gx = add(gx, mul(mul(SH_C36, sub(mul(3.0f, q.xx), mul(3.0f, q.yy))), s[15]));
        gy = add(gy, mul(mul(SH_C36, mul(-6.0f, q.xy)), s[15]));
    }
}

// colour + sum over 1 <= k < Ka of B[k] row[k - 1], per channel, before the clamp
template <int L>
__device__ __forceinline__ void sh_sum(const float (&B)[ShShape<L>::K], const float* row, int Ka, const float* __restrict__ colour, float (&c)[3]) {
    c[0] = colour[0]; c[1] = colour[1]; c[2] = colour[2];
#pragma unroll
    for (int k = 1; k < ShShape<L>::K; ++k) {
        if (k < Ka) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = add(c[ch], mul(B[k], row[3 * (k - 1) + ch]));
        }
    }
}

// One view's backward: the colour gradient g of a (view, Gaussian) through the clamp (ge), the basis B at the view's direction, and dv,
// what reaches the Gaussian's position through the normalisation of the direction.  gauss_sh_bwd adds ge, B ge and dv over the views;
// gauss_sh_pose_bwd takes dv on to the view's matrix (§28).
template <int L>
struct ShViewBwd {
    float ge[3], B[ShShape<L>::K], dv[3];
};

template <int L>
__device__ __forceinline__ void sh_view_bwd(const float* __restrict__ m, const ShPoint& p, const float* row, int Ka,
                                            const float* __restrict__ colour, const float (&g)[3], ShViewBwd<L>& o) {
    constexpr int K = ShShape<L>::K;
    const ShDir d = sh_direction(m, p);
    float c[3], s[K];
    sh_basis<L>(d, o.B);
    sh_sum<L>(o.B, row, Ka, colour, c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o.ge[ch] = c[ch] < 0.0f ? 0.0f : g[ch];  // where the clamp cut, nothing passes
    s[0] = 0.0f;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        s[k] = 0.0f;
        if (k < Ka) {
            const float* r = row + 3 * (k - 1);
            s[k] = add(add(mul(o.ge[0], r[0]), mul(o.ge[1], r[1])), mul(o.ge[2], r[2]));
        }
    }
    float ax, ay, az;
    sh_basis_grad<L>(d, s, ax, ay, az);
    const float dot = add(add(mul(d.x, ax), mul(d.y, ay)), mul(d.z, az));
    o.dv[0] = dvd(sub(ax, mul(d.x, dot)), d.len);
    o.dv[1] = dvd(sub(ay, mul(d.y, dot)), d.len);
    o.dv[2] = dvd(sub(az, mul(d.z, dot)), d.len);
}

// ------------------------------------------------------------------------------------------------ the kernels
// grid: (workgroups of 256 Gaussians, views).  A workgroup none of whose Gaussians the view draws reads no coefficients.
template <int L>
__global__ __launch_bounds__(256) void gauss_sh_colour_kernel(const u32x4* __restrict__ pts, const int32_t* __restrict__ ids,
                                                               const float* __restrict__ mats, int64_t n, int nmat,
                                                               const int32_t* __restrict__ count, const float* __restrict__ colour,
                                                               const float* __restrict__ sh, int active, float* __restrict__ colours) {
    __shared__ __attribute__((aligned(16))) float rows[256 * ShShape<L>::PAD];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    const bool live = idx < n;
    const int64_t o = view * n + (live ? idx : 0);
    const bool drawn = live && count[o] > 0;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (__syncthreads_or(drawn)) {
        stage_rows<L>(sh, n, rows);
        if (drawn) {
            const ShPoint p = sh_point(pts, ids, nmat, idx);
            const ShDir d = sh_direction(mats + (view * nmat + p.id) * 12, p);
            float B[ShShape<L>::K];
            sh_basis<L>(d, B);
            sh_sum<L>(B, rows + threadIdx.x * ShShape<L>::PAD, (active + 1) * (active + 1), colour + 3 * idx, c);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] < 0.0f ? 0.0f : c[ch];
        }
    }
    if (live) {
        colours[3 * o] = c[0]; colours[3 * o + 1] = c[1]; colours[3 * o + 2] = c[2];
    }
}

template <int L>
__global__ __launch_bounds__(256) void gauss_sh_bwd_kernel(const u32x4* __restrict__ pts, const int32_t* __restrict__ ids,
                                                            const float* __restrict__ mats, int64_t n, int V, int nmat,
                                                            const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                            const float* __restrict__ partial, int64_t E, const float* __restrict__ colour,
                                                            const float* __restrict__ sh, int active, float* __restrict__ d_colour,
                                                            float* __restrict__ d_sh, float* __restrict__ d_xyz) {
    constexpr int K = ShShape<L>::K, ROW = ShShape<L>::ROW, PAD = ShShape<L>::PAD;
    __shared__ __attribute__((aligned(16))) float rows[256 * PAD];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < n;
    stage_rows<L>(sh, n, rows);
    float* row = rows + threadIdx.x * PAD;
    const int Ka = (active + 1) * (active + 1);
    float gsh[ROW], gc[3] = {0.0f, 0.0f, 0.0f}, gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
    for (int j = 0; j < ROW; ++j) gsh[j] = 0.0f;
    if (live) {
        const ShPoint p = sh_point(pts, ids, nmat, idx);
        int view = 0;
        const auto chain = [&](const float (&g)[3]) {                      // the view's colour gradient through the rule
            ShViewBwd<L> b;
            sh_view_bwd<L>(mats + ((int64_t)view * nmat + p.id) * 12, p, row, Ka, colour + 3 * idx, g, b);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) gc[ch] = add(gc[ch], b.ge[ch]);
#pragma unroll
            for (int k = 1; k < K; ++k) {
                if (k < Ka) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) gsh[3 * (k - 1) + ch] = add(gsh[3 * (k - 1) + ch], mul(b.B[k], b.ge[ch]));
                }
            }
            gx = add(gx, b.dv[0]);
            gy = add(gy, b.dv[1]);
            gz = add(gz, b.dv[2]);
        };
        for (; view < V; ++view) with_partials<SUM_COLOUR, 3>(partial, count, offsets, (int64_t)view * n + idx, E, chain);
    }
    __syncthreads();                                                        // every lane has read its coefficients
#pragma unroll
    for (int j = 0; j < ROW; ++j) row[j] = gsh[j];
    store_rows<L>(rows, n, d_sh);
    if (live) {
        d_colour[3 * idx] = gc[0]; d_colour[3 * idx + 1] = gc[1]; d_colour[3 * idx + 2] = gc[2];
        d_xyz[3 * idx] = gx; d_xyz[3 * idx + 1] = gy; d_xyz[3 * idx + 2] = gz;
    }
}

// §28: what the direction says about the view's matrices.  grid: (chunks of 256 Gaussians, views), a lane per (view, Gaussian); the
// coefficients staged as above, the twelve values reduced per matrix id as gauss_pose_bwd reduces its own (pose_reduce).
template <int L>
__global__ __launch_bounds__(256) void gauss_sh_pose_bwd_kernel(const u32x4* __restrict__ pts, const int32_t* __restrict__ ids,
                                                                 const float* __restrict__ mats, int64_t n, int nmat,
                                                                 const int32_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                                 const float* __restrict__ partial, int64_t E, const float* __restrict__ colour,
                                                                 const float* __restrict__ sh, int active, float* __restrict__ stage) {
    __shared__ __attribute__((aligned(16))) float rows[256 * ShShape<L>::PAD];
    __shared__ PoseScratch lds;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    const bool live = idx < n;
    float g[POSE_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool drawn = false;
    int id = 0;
    if (!__syncthreads_or(live && count[view * n + idx] > 0)) return;       // the same for every lane: stage keeps the entry point's zeros
    stage_rows<L>(sh, n, rows);
    if (live) {
        with_partials<SUM_COLOUR, 3>(partial, count, offsets, view * n + idx, E, [&](const float (&up)[3]) {
            const ShPoint p = sh_point(pts, ids, nmat, idx);
            const float* m = mats + (view * nmat + p.id) * 12;
            ShViewBwd<L> b;
            sh_view_bwd<L>(m, p, rows + threadIdx.x * ShShape<L>::PAD, (active + 1) * (active + 1), colour + 3 * idx, up, b);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int k = 0; k < 3; ++k) g[4 * r + k] = mul(b.dv[k], m[4 * r + 3]);
                g[4 * r + 3] = add(add(mul(b.dv[0], m[4 * r]), mul(b.dv[1], m[4 * r + 1])), mul(b.dv[2], m[4 * r + 2]));
            }
            id = p.id;
            drawn = true;
        });
    }
    pose_reduce(g, drawn, id, nmat, stage + view * nmat * pose_chunks(n) * POSE_SUMS, pose_chunks(n), lds);
}

int check_sh(const char* name, int64_t n, int V, int nmat, const int32_t* ids, int degree, int active) {
    MUDG_REQUIRE(n > 0 && V > 0, "%s: %lld Gaussians in %d views", name, (long long)n, V);
    MUDG_REQUIRE(n <= 0x7fffffffLL, "%s: %lld Gaussians (the sorted value is a 32-bit index)", name, (long long)n);
    MUDG_REQUIRE(nmat > 0, "%s: %d matrices per view", name, nmat);
    MUDG_REQUIRE(ids || nmat == 1, "%s: %d matrices per view need per-point ids", name, nmat);
    MUDG_REQUIRE(degree >= 1 && degree <= 3, "%s: harmonics of degree %d (1, 2 or 3)", name, degree);
    MUDG_REQUIRE(active >= 0 && active <= degree, "%s: active degree %d of %d", name, active, degree);
    MUDG_REQUIRE(grid_ok(n), "%s: %lld Gaussians are more workgroups than a grid holds", name, (long long)n);
    return MUDG_OK;
}

}  // namespace

extern "C" int mudg_gauss_sh_colour(const void* points, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, const int32_t* count,
                                    const float* colour, const float* sh, int degree, int active, float* colours, void* stream) {
    MUDG_REQUIRE(points && mats && count && colour && sh && colours, "mudg_gauss_sh_colour: null argument");
    MUDG_REQUIRE(aligned16(points) && aligned16(sh), "mudg_gauss_sh_colour: unaligned points or coefficients");
    if (const int e = check_sh("mudg_gauss_sh_colour", n, V, nmat, ids, degree, active)) return e;
    MUDG_REQUIRE(V <= 65535, "mudg_gauss_sh_colour: %d views (the grid's second axis holds 65535)", V);
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)V);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u32x4* pts = reinterpret_cast<const u32x4*>(points);
    if (degree == 1) hipLaunchKernelGGL(gauss_sh_colour_kernel<1>, grid, dim3(256), 0, s, pts, ids, mats, n, nmat, count, colour, sh, active, colours);
    else if (degree == 2) hipLaunchKernelGGL(gauss_sh_colour_kernel<2>, grid, dim3(256), 0, s, pts, ids, mats, n, nmat, count, colour, sh, active, colours);
    else hipLaunchKernelGGL(gauss_sh_colour_kernel<3>, grid, dim3(256), 0, s, pts, ids, mats, n, nmat, count, colour, sh, active, colours);
    return mudg_check_launch("mudg_gauss_sh_colour");
}

extern "C" int mudg_gauss_sh_bwd(const void* points, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, const int32_t* count,
                                 const int64_t* offsets, const float* partial, int64_t E, const float* colour, const float* sh, int degree,
                                 int active, float* d_colour, float* d_sh, float* d_xyz_dir, void* stream) {
    MUDG_REQUIRE(points && mats && count && offsets && partial && colour && sh && d_colour && d_sh && d_xyz_dir, "mudg_gauss_sh_bwd: null argument");
    MUDG_REQUIRE(aligned16(points) && aligned16(sh) && aligned16(d_sh), "mudg_gauss_sh_bwd: unaligned points or coefficients");
    MUDG_REQUIRE(aligned8(offsets), "mudg_gauss_sh_bwd: unaligned offsets");
    if (const int e = check_sh("mudg_gauss_sh_bwd", n, V, nmat, ids, degree, active)) return e;
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_sh_bwd: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u32x4* pts = reinterpret_cast<const u32x4*>(points);
    if (degree == 1)
        hipLaunchKernelGGL(gauss_sh_bwd_kernel<1>, grid, dim3(256), 0, s, pts, ids, mats, n, V, nmat, count, offsets, partial, E, colour, sh, active,
                           d_colour, d_sh, d_xyz_dir);
    else if (degree == 2)
        hipLaunchKernelGGL(gauss_sh_bwd_kernel<2>, grid, dim3(256), 0, s, pts, ids, mats, n, V, nmat, count, offsets, partial, E, colour, sh, active,
                           d_colour, d_sh, d_xyz_dir);
    else
        hipLaunchKernelGGL(gauss_sh_bwd_kernel<3>, grid, dim3(256), 0, s, pts, ids, mats, n, V, nmat, count, offsets, partial, E, colour, sh, active,
                           d_colour, d_sh, d_xyz_dir);
    return mudg_check_launch("mudg_gauss_sh_bwd");
}

extern "C" int mudg_gauss_sh_pose_bwd(const void* points, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, const int32_t* count,
                                      const int64_t* offsets, const float* partial, int64_t E, const float* colour, const float* sh, int degree,
                                      int active, float* stage, float* d_mats_dir, void* stream) {
    MUDG_REQUIRE(points && mats && count && offsets && partial && colour && sh && stage && d_mats_dir, "mudg_gauss_sh_pose_bwd: null argument");
    MUDG_REQUIRE(aligned16(points) && aligned16(sh), "mudg_gauss_sh_pose_bwd: unaligned points or coefficients");
    MUDG_REQUIRE(aligned8(offsets), "mudg_gauss_sh_pose_bwd: unaligned offsets");
    if (const int e = check_sh("mudg_gauss_sh_pose_bwd", n, V, nmat, ids, degree, active)) return e;
    MUDG_REQUIRE(V <= 65535, "mudg_gauss_sh_pose_bwd: %d views (the grid's second axis holds 65535)", V);
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_sh_pose_bwd: %lld entries (1 .. 2^31 - 1)", (long long)E);
    const dim3 grid((unsigned)pose_chunks(n), (unsigned)V);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u32x4* pts = reinterpret_cast<const u32x4*>(points);
    if (!pose_clear(stage, n, V, nmat, s)) return mudg_check_launch("mudg_gauss_sh_pose_bwd");
    if (degree == 1)
        hipLaunchKernelGGL(gauss_sh_pose_bwd_kernel<1>, grid, dim3(256), 0, s, pts, ids, mats, n, nmat, count, offsets, partial, E, colour, sh, active,
                           stage);
    else if (degree == 2)
        hipLaunchKernelGGL(gauss_sh_pose_bwd_kernel<2>, grid, dim3(256), 0, s, pts, ids, mats, n, nmat, count, offsets, partial, E, colour, sh, active,
                           stage);
    else
        hipLaunchKernelGGL(gauss_sh_pose_bwd_kernel<3>, grid, dim3(256), 0, s, pts, ids, mats, n, nmat, count, offsets, partial, E, colour, sh, active,
                           stage);
    pose_finish(stage, n, V, nmat, d_mats_dir, s);
    return mudg_check_launch("mudg_gauss_sh_pose_bwd");
}
