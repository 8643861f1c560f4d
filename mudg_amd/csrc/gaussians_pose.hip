// gaussians_pose.hip — the gradient of the Gaussian splat renderer's matrices: what a loss on the images says about
// mats (V, nmat, 12), for camera and object-pose refinement.
//   gauss_pose_bwd  a lane owns a (view, Gaussian): it sums the Gaussian's partials (§24) in ascending order, recomputes the forward's
//                   projection bit for bit (gauss_view), takes the sums through the chain rule that gauss_project_bwd uses (gauss_view_bwd)
//                   and forms the twelve contributions to its matrix.  A workgroup of 256 consecutive Gaussians reduces them once per
//                   matrix id present (pose_reduce) into a stage buffer; a finishing workgroup per (view, matrix) adds the chunks
//                   (pose_finish_kernel).  Plain stores, fixed orders, no atomics
// Everything is fp32, each operation a single rounded one in the order DESIGN.md §28 writes it, so d_mats is bit-equal to the numpy
// definition in tests/gaussians_pose_reference.py and a repeat run gives the same bits.  No MFMA operand is touched.
#include "gauss_shared.h"

namespace {

// grid: (chunks of 256 Gaussians, views)
__global__ __launch_bounds__(256) void gauss_pose_bwd_kernel(const u32x4* __restrict__ pts, const float* __restrict__ cov,
                                                              const int32_t* __restrict__ ids, const float* __restrict__ mats, int64_t n,
                                                              int nmat, int H, int W, GaussCam cam, const int32_t* __restrict__ count,
                                                              const int64_t* __restrict__ offsets, const float* __restrict__ partial,
                                                              int64_t E, float* __restrict__ stage) {
    __shared__ PoseScratch lds;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    float g[POSE_SUMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool drawn = false;
    int id = 0;
    if (idx < n) {
        with_partials<0, GAUSS_SUMS>(partial, count, offsets, view * n + idx, E, [&](const float (&acc)[GAUSS_SUMS]) {
            const GaussPoint p = load_gaussian(pts, cov, ids, nmat, idx);
            const float* m = mats + (view * nmat + p.id) * 12;
            GaussView w;                                                    // the forward's values (§23 steps 2 - 9)
            if (!gauss_view(m, p, cam, gauss_limit(W, cam.fx), gauss_limit(H, cam.fy), w)) return;
            GaussViewBwd b;
            gauss_view_bwd(m, w, cam, acc, b);
            const float xyz[3] = {p.x, p.y, p.z};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                g[k] = add(mul(b.dxc, xyz[k]), mul(b.dt0[k], w.j00));
                g[4 + k] = add(mul(b.dyc, xyz[k]), mul(b.dt1[k], w.j11));
                g[8 + k] = add(mul(b.dzc, xyz[k]), add(mul(b.dt0[k], w.j02), mul(b.dt1[k], w.j12)));
            }
            g[3] = b.dxc; g[7] = b.dyc; g[11] = b.dzc;
            id = p.id;
            drawn = true;
        });
    }
    pose_reduce(g, drawn, id, nmat, stage + view * nmat * pose_chunks(n) * POSE_SUMS, pose_chunks(n), lds);
}

}  // namespace

extern "C" int mudg_gauss_pose_bwd(const void* points, const float* cov, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, int H,
                                   int W, float fx, float fy, float cx, float cy, float znear, float zfar, const int32_t* count,
                                   const int64_t* offsets, const float* partial, int64_t E, float* stage, float* d_mats, void* stream) {
    MUDG_REQUIRE(points && cov && mats && count && offsets && partial && stage && d_mats, "mudg_gauss_pose_bwd: null argument");
    MUDG_REQUIRE(aligned16(points), "mudg_gauss_pose_bwd: unaligned points");
    MUDG_REQUIRE(aligned8(offsets), "mudg_gauss_pose_bwd: unaligned offsets");
    MUDG_REQUIRE(nmat > 0, "mudg_gauss_pose_bwd: %d matrices per view", nmat);
    if (const int e = check_views("mudg_gauss_pose_bwd", n, V, H, W)) return e;
    MUDG_REQUIRE(V <= 65535, "mudg_gauss_pose_bwd: %d views (the grid's second axis holds 65535)", V);
    MUDG_REQUIRE(ids || nmat == 1, "mudg_gauss_pose_bwd: %d matrices per view need per-point ids", nmat);
    MUDG_REQUIRE(grid_ok(n), "mudg_gauss_pose_bwd: %lld Gaussians are more workgroups than a grid holds", (long long)n);
    MUDG_REQUIRE(entries_ok(E), "mudg_gauss_pose_bwd: %lld entries (1 .. 2^31 - 1)", (long long)E);
    if (const int e = check_camera("mudg_gauss_pose_bwd", fx, fy, cx, cy, znear, zfar)) return e;
    const GaussCam cam = {fx, fy, cx, cy, znear, zfar};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!pose_clear(stage, n, V, nmat, s)) return mudg_check_launch("mudg_gauss_pose_bwd");
    hipLaunchKernelGGL(gauss_pose_bwd_kernel, dim3((unsigned)pose_chunks(n), (unsigned)V), dim3(256), 0, s, reinterpret_cast<const u32x4*>(points),
                       cov, ids, mats, n, nmat, H, W, cam, count, offsets, partial, E, stage);
    pose_finish(stage, n, V, nmat, d_mats, s);
    return mudg_check_launch("mudg_gauss_pose_bwd");
}
