// optim.hip — what the training step does AFTER the backward pass (reference: lvdm/models/ddpm3d.py:1267-1300 configure_optimizers
// -> AdamW, lvdm/ema.py LitEma, the trainer's gradient_clip_val and precision: 16): AdamW, the averaged weights and their
// exchange, gradient-norm clipping and the loss scaler.  Everything works on fp32 tensors through chunk tables: int64 rows of
// (address of each operand's chunk ..., count), at most CLIP_CHUNK values per row, one 256-thread workgroup per row — one launch
// for the UNet's 1520 tensors.  There is ONE walk over a row (multi_walk), ONE AdamW expression (adamw_elem), ONE average
// (ema_elem) and ONE fp64 block sum (block_sum_256); the kernels are those four put together, which is what keeps them
// bit-equal to each other.  Every reduction has a fixed order: no atomics.
#include "common.h"

namespace {

constexpr int CLIP_CHUNK = 16384;

// ---------------------------------------------------------------------------------------------------- the walk
// Pure streaming: a chunk is walked in pieces of 256 x 16 bytes per operand, MT_U pieces at a time, every load of the pieces
// issued before the first use (the updates are in place, so the compiler may not move a load above a store by itself); a chunk
// whose addresses are not all 16-byte aligned (a view into a flat bucket) and the last count % 4 values take the scalar loop.
// row = NP addresses, then the count.  op(x) sees one element of each operand in x[0 .. NP); the operands named by the bit mask
// Op::WRITES are stored back.
constexpr int MT_U = 2;
// The addresses come out of the table as integers: typed as global memory, so that the accesses are global_* and not flat_* ones.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

template <int NP, class Op>
__device__ __forceinline__ void multi_walk(const int64_t* row, const Op& op) {
    int64_t any = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) any |= row[k];
    const int n = (int)row[NP];
    int done = 0;
    if ((any & 15) == 0) {
        const int n4 = n >> 2;
        for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * MT_U) {
            f32x4 x[MT_U][NP] = {};
#pragma unroll
            for (int u = 0; u < MT_U; ++u) if (i0 + 256 * u < n4) {
#pragma unroll
                for (int k = 0; k < NP; ++k) x[u][k] = reinterpret_cast<const gf32x4*>(row[k])[i0 + 256 * u];
            }
#pragma unroll
            for (int u = 0; u < MT_U; ++u) if (i0 + 256 * u < n4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float y[NP];
#pragma unroll
                    for (int k = 0; k < NP; ++k) y[k] = x[u][k][e];
                    op(y);
#pragma unroll
                    for (int k = 0; k < NP; ++k) x[u][k][e] = y[k];
                }
#pragma unroll
                for (int k = 0; k < NP; ++k) if (Op::WRITES >> k & 1) reinterpret_cast<gf32x4*>(row[k])[i0 + 256 * u] = x[u][k];
            }
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += 256) {
        float y[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) y[k] = reinterpret_cast<const gfloat*>(row[k])[i];
        op(y);
#pragma unroll
        for (int k = 0; k < NP; ++k) if (Op::WRITES >> k & 1) reinterpret_cast<gfloat*>(row[k])[i] = y[k];
    }
}

// ---------------------------------------------------------------------------------------------- averaged weights
// The exponential moving average of the weights (lvdm/ema.py LitEma.forward) and the weight exchange of ema_scope
// (ddpm3d.py:188-201).
//   shadow <- shadow - one_minus_decay * (shadow - param), each operation rounded on its own: the bits of the reference on the CPU
__device__ __forceinline__ float ema_elem(float s, float p, float omd) { return __fsub_rn(s, __fmul_rn(omd, __fsub_rn(s, p))); }

struct EmaOp {                                   // rows (shadow, param, count)
    static constexpr unsigned WRITES = 1;
    float omd;
    __device__ __forceinline__ void operator()(float (&x)[2]) const { x[0] = ema_elem(x[0], x[1], omd); }
};
__global__ __launch_bounds__(256) void ema_multi_kernel(const int64_t* __restrict__ table, float omd) {
    multi_walk<2>(table + 3 * (int64_t)blockIdx.x, EmaOp{omd});
}

struct SwapOp {                                  // rows (a, b, count): the two tensors change places; nothing else is held
    static constexpr unsigned WRITES = 3;
    __device__ __forceinline__ void operator()(float (&x)[2]) const { const float a = x[0]; x[0] = x[1]; x[1] = a; }
};
__global__ __launch_bounds__(256) void swap_multi_kernel(const int64_t* __restrict__ table) {
    multi_walk<2>(table + 3 * (int64_t)blockIdx.x, SwapOp{});
}

// ---------------------------------------------------------------------------------------------------------- AdamW
// torch.optim.AdamW semantics (decoupled weight decay): fp32 parameters, gradients and moments, in place.
//   step = lr / (1 - b1^n), decay = 1 - lr wd, bc2 = 1 - b2^n
struct AdamWStep { float b1, b2, eps, bc2, step, decay; };
// For the n-th step: computed on the host by the plain forms, per workgroup on the device (n out of the scaler's record) by the
// scaled ones.
__host__ __device__ inline AdamWStep adamw_step(float lr, float b1, float b2, float eps, float wd, float n) {
    return {b1, b2, eps, 1.0f - powf(b2, n), lr / (1.0f - powf(b1, n)), 1.0f - lr * wd};
}
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamWStep& a) {
    const float pi = p * a.decay;
    const float mi = a.b1 * m + (1.0f - a.b1) * g;
    const float vi = a.b2 * v + (1.0f - a.b2) * g * g;
    m = mi; v = vi;
    const float denom = sqrtf(vi) / sqrtf(a.bc2) + a.eps;
    p = pi - a.step * (mi / denom);
}

// One tensor, one element per thread: the per-tensor fallback of AdamW.step and the yardstick of the bit tests.
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                             AdamWStep a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float pe = p[i], me = m[i], ve = v[i];
    adamw_elem(pe, g[i], me, ve, a);
    p[i] = pe; m[i] = me; v[i] = ve;
}

// Rows (p, g, m, v, count), or with NP = 5 (p, g, m, v, shadow, count): the average then reads the new parameter value out of the
// register it was just computed in — one read and one write of the shadow on top of the AdamW traffic, no second read of the
// parameter.  The gradient is taken as (g * inv) * coef, each product rounded on its own (the scaled forms; see loss scaling).
template <int NP, bool SCALED>
struct AdamWOp {
    static constexpr unsigned WRITES = NP == 5 ? 0x1d : 0xd;
    AdamWStep a;
    float omd, inv, coef;
    __device__ __forceinline__ void operator()(float (&x)[NP]) const {
        adamw_elem(x[0], SCALED ? __fmul_rn(__fmul_rn(x[1], inv), coef) : x[1], x[2], x[3], a);
        if constexpr (NP == 5) x[4] = ema_elem(x[4], x[0], omd);
    }
};
__global__ __launch_bounds__(256) void adamw_multi_kernel(const int64_t* __restrict__ table, AdamWStep a) {
    multi_walk<4>(table + 5 * (int64_t)blockIdx.x, AdamWOp<4, false>{a, 0.f, 1.f, 1.f});
}
__global__ __launch_bounds__(256) void adamw_ema_multi_kernel(const int64_t* __restrict__ table, AdamWStep a, float omd) {
    multi_walk<5>(table + 6 * (int64_t)blockIdx.x, AdamWOp<5, false>{a, omd, 1.f, 1.f});
}

// Global gradient norm and clipping over many tensors without a host round trip (torch.nn.utils.clip_grad_norm_ semantics: the
// reference's trainer clips to norm 0.5).  `table` lists chunks as (address, count) pairs; one workgroup sums the squares of a
// chunk in fp64 (fixed order), one workgroup then folds the chunk sums in order and writes out[0] = the norm,
// out[1] = min(1, max_norm / (norm + 1e-6)); the scale pass multiplies every chunk by out[1].
//
// ------------------------------------------------------------------------------------------------- loss scaling
// torch.amp.GradScaler on the device (fp16 training: the loss is multiplied by `scale` before backward, so that output gradients
// below the operand type's range survive the operand rounding).  The state is one 16-byte record
//   [0] float scale   [1] int growth tracker   [2] int overflow flag of the current step   [3] int count of steps actually taken
// which only kernels read and write: nothing in a step depends on a value the host would have to fetch.
//   chunk_sumsq<true> / norm_fold with the record   the norm pass of the SCALED gradients: per chunk the fp64 sum of
//                    (double)(g * inv_scale)^2 with inv_scale = float(1 / double(scale)) (torch's unscale_); the fold writes
//                    out[0] = the unscaled norm, out[1] = the clip coefficient (1 when max_norm <= 0: no clipping asked for) and the
//                    overflow flag: the sum of squares of finite fp32 values cannot overflow fp64, so the step has overflowed iff the
//                    folded sum is not finite (any +-inf or NaN gradient makes it so).  The gradients are NOT written.
//   adamw_scaled_*   adamw_multi_kernel / adamw_ema_multi_kernel on the gradient (g * inv_scale) * coef (the bits of unscale_
//                    followed by clip_grad_norm_); flag set: parameter and moments are neither changed nor rewritten (the EMA form
//                    still averages the unchanged parameter, as LitEma.forward does after a skipped step); the bias corrections use
//                    n = count + 1.
//   loss_scale_update   torch's _amp_update_scale_, then count += !flag and the flag is cleared.
struct ScaleRecord { float scale; int tracker; int overflow; int taken; };
__device__ __forceinline__ float inv_scale_of(float scale) { return (float)(1.0 / (double)scale); }

// The sum over a 256-thread workgroup, the same tree everywhere (the bits of the norm depend on it): every thread's value to LDS,
// then the widths 128 .. 1 folded with a barrier between each.
__device__ __forceinline__ double block_sum_256(double s) {
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

template <bool SCALED>                           // SCALED: the squares are those of g * inv_scale (rec is read only then)
__global__ __launch_bounds__(256) void chunk_sumsq_kernel(const int64_t* __restrict__ table, double* __restrict__ partial,
                                                           const ScaleRecord* __restrict__ rec) {
    const float inv = SCALED ? inv_scale_of(rec->scale) : 1.0f;
    const float* x = reinterpret_cast<const float*>(table[2 * blockIdx.x]);
    const int n = (int)table[2 * blockIdx.x + 1];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { const double v = (double)(SCALED ? __fmul_rn(x[i], inv) : x[i]); s += v * v; }
    s = block_sum_256(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// rec null: clip_grad_norm_ (max_norm > 0 is the caller's).  rec given: max_norm <= 0 asks for no clipping, and the flag is written.
__global__ __launch_bounds__(256) void norm_fold_kernel(const double* __restrict__ partial, int nchunks, float max_norm, float* __restrict__ out,
                                                         ScaleRecord* __restrict__ rec) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 256) s += partial[i];
    const double total = block_sum_256(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        out[0] = norm;
        const float coef = max_norm / (norm + 1e-6f);
        out[1] = ((!rec || max_norm > 0.f) && coef < 1.0f) ? coef : 1.0f;
        if (rec) rec->overflow = __builtin_isfinite(total) ? 0 : 1;
    }
}
__global__ __launch_bounds__(256) void chunk_scale_kernel(const int64_t* __restrict__ table, const float* __restrict__ out) {
    const float coef = out[1];
    if (coef == 1.0f) return;
    float* x = reinterpret_cast<float*>(table[2 * blockIdx.x]);
    const int n = (int)table[2 * blockIdx.x + 1];
    for (int i = threadIdx.x; i < n; i += 256) x[i] *= coef;
}
// scaler.unscale_: g <- g * inv_scale in place, for callers who want to look at the gradients (the optimiser does not need it).
__global__ __launch_bounds__(256) void unscale_kernel(const int64_t* __restrict__ table, const ScaleRecord* __restrict__ rec) {
    const float inv = inv_scale_of(rec->scale);
    float* x = reinterpret_cast<float*>(table[2 * blockIdx.x]);
    const int n = (int)table[2 * blockIdx.x + 1];
    for (int i = threadIdx.x; i < n; i += 256) x[i] = __fmul_rn(x[i], inv);
}

// What a workgroup of the scaled optimiser reads once (uniform addresses of read-only memory: scalar loads).
template <int NP>
__device__ __forceinline__ AdamWOp<NP, true> scaled_op(const ScaleRecord* __restrict__ rec, const float* __restrict__ stat, float lr, float b1,
                                                       float b2, float eps, float wd, float omd) {
    return {adamw_step(lr, b1, b2, eps, wd, (float)(rec->taken + 1)), omd, inv_scale_of(rec->scale), stat[1]};
}

__global__ __launch_bounds__(256) void adamw_scaled_multi_kernel(const int64_t* __restrict__ table, float lr, float b1, float b2, float eps,
                                                                  float wd, const ScaleRecord* __restrict__ rec, const float* __restrict__ stat) {
    if (rec->overflow != 0) return;                                    // overflow: nothing is rewritten
    multi_walk<4>(table + 5 * (int64_t)blockIdx.x, scaled_op<4>(rec, stat, lr, b1, b2, eps, wd, 0.f));
}

// A skipped step moves the shadow towards the unchanged parameter: the average alone, over (shadow, p) of the row.
__global__ __launch_bounds__(256) void adamw_scaled_ema_multi_kernel(const int64_t* __restrict__ table, float lr, float b1, float b2, float eps,
                                                                      float wd, float omd, const ScaleRecord* __restrict__ rec,
                                                                      const float* __restrict__ stat) {
    const int64_t* row = table + 6 * (int64_t)blockIdx.x;
    if (rec->overflow != 0) {
        const int64_t view[3] = {row[4], row[0], row[5]};
        multi_walk<2>(view, EmaOp{omd});
        return;
    }
    multi_walk<5>(row, scaled_op<5>(rec, stat, lr, b1, b2, eps, wd, omd));
}

__global__ void loss_scale_update_kernel(ScaleRecord* __restrict__ rec, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int flag = rec->overflow;
    if (flag) {
        rec->scale = __fmul_rn(rec->scale, backoff);
        rec->tracker = 0;
    } else {
        const int good = rec->tracker + 1;
        if (good == interval) {
            const float grown = __fmul_rn(rec->scale, growth);
            if (__builtin_isfinite(grown)) rec->scale = grown;               // a growth that would leave fp32 is refused
            rec->tracker = 0;
        } else {
            rec->tracker = good;
        }
    }
    rec->taken += flag ? 0 : 1;
    rec->overflow = 0;
}

inline hipStream_t hs(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

}  // namespace

extern "C" {

int mudg_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
               void* stream) {
    MUDG_REQUIRE(p && g && m && v && n > 0 && step > 0, "mudg_adamw: bad arguments");
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs(stream), p, g, m, v, n,
                       adamw_step(lr, beta1, beta2, eps, weight_decay, (float)step));
    return mudg_check_launch("mudg_adamw");
}

int mudg_adamw_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream) {
    MUDG_REQUIRE(table && nchunks > 0 && step > 0, "mudg_adamw_multi: bad arguments");
    hipLaunchKernelGGL(adamw_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table,
                       adamw_step(lr, beta1, beta2, eps, weight_decay, (float)step));
    return mudg_check_launch("mudg_adamw_multi");
}

int mudg_adamw_ema_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         float one_minus_decay, void* stream) {
    MUDG_REQUIRE(table && nchunks > 0 && step > 0, "mudg_adamw_ema_multi: bad arguments");
    MUDG_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "mudg_adamw_ema_multi: one_minus_decay=%g outside [0, 1]", (double)one_minus_decay);
    hipLaunchKernelGGL(adamw_ema_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table,
                       adamw_step(lr, beta1, beta2, eps, weight_decay, (float)step), one_minus_decay);
    return mudg_check_launch("mudg_adamw_ema_multi");
}

int mudg_ema_multi(const int64_t* table, int nchunks, float one_minus_decay, void* stream) {
    MUDG_REQUIRE(table && nchunks > 0, "mudg_ema_multi: bad arguments");
    MUDG_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "mudg_ema_multi: one_minus_decay=%g outside [0, 1]", (double)one_minus_decay);
    hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, one_minus_decay);
    return mudg_check_launch("mudg_ema_multi");
}

int mudg_swap_multi(const int64_t* table, int nchunks, void* stream) {
    MUDG_REQUIRE(table && nchunks > 0, "mudg_swap_multi: bad arguments");
    hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table);
    return mudg_check_launch("mudg_swap_multi");
}

int mudg_clip_chunk(void) { return CLIP_CHUNK; }

int mudg_clip_grad_norm(const int64_t* table, int nchunks, double* partial, float max_norm, float* out, void* stream) {
    MUDG_REQUIRE(table && partial && out && nchunks > 0 && max_norm > 0.f, "mudg_clip_grad_norm: bad arguments");
    hipLaunchKernelGGL(chunk_sumsq_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, partial, nullptr);
    hipLaunchKernelGGL(norm_fold_kernel, dim3(1), dim3(256), 0, hs(stream), partial, nchunks, max_norm, out, nullptr);
    hipLaunchKernelGGL(chunk_scale_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, out);
    return mudg_check_launch("mudg_clip_grad_norm");
}

int mudg_scaled_grad_norm(const int64_t* table, int nchunks, double* partial, float max_norm, float* out, void* record, void* stream) {
    MUDG_REQUIRE(table && partial && out && record && nchunks > 0 && max_norm >= 0.f, "mudg_scaled_grad_norm: bad arguments");
    MUDG_REQUIRE((reinterpret_cast<uintptr_t>(record) & 15u) == 0, "mudg_scaled_grad_norm: the scaler record must be 16-byte aligned");
    ScaleRecord* rec = reinterpret_cast<ScaleRecord*>(record);
    hipLaunchKernelGGL(chunk_sumsq_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, partial, rec);
    hipLaunchKernelGGL(norm_fold_kernel, dim3(1), dim3(256), 0, hs(stream), partial, nchunks, max_norm, out, rec);
    return mudg_check_launch("mudg_scaled_grad_norm");
}

int mudg_unscale_multi(const int64_t* table, int nchunks, const void* record, void* stream) {
    MUDG_REQUIRE(table && record && nchunks > 0, "mudg_unscale_multi: bad arguments");
    hipLaunchKernelGGL(unscale_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, reinterpret_cast<const ScaleRecord*>(record));
    return mudg_check_launch("mudg_unscale_multi");
}

int mudg_adamw_scaled_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, const void* record,
                            const float* stat, void* stream) {
    MUDG_REQUIRE(table && record && stat && nchunks > 0, "mudg_adamw_scaled_multi: bad arguments");
    hipLaunchKernelGGL(adamw_scaled_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, lr, beta1, beta2, eps, weight_decay,
                       reinterpret_cast<const ScaleRecord*>(record), stat);
    return mudg_check_launch("mudg_adamw_scaled_multi");
}

int mudg_adamw_scaled_ema_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                                float one_minus_decay, const void* record, const float* stat, void* stream) {
    MUDG_REQUIRE(table && record && stat && nchunks > 0, "mudg_adamw_scaled_ema_multi: bad arguments");
    MUDG_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "mudg_adamw_scaled_ema_multi: one_minus_decay=%g outside [0, 1]",
                 (double)one_minus_decay);
    hipLaunchKernelGGL(adamw_scaled_ema_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, hs(stream), table, lr, beta1, beta2, eps, weight_decay,
                       one_minus_decay, reinterpret_cast<const ScaleRecord*>(record), stat);
    return mudg_check_launch("mudg_adamw_scaled_ema_multi");
}

int mudg_loss_scale_update(void* record, float growth_factor, float backoff_factor, int growth_interval, void* stream) {
    MUDG_REQUIRE(record && growth_factor > 1.f && backoff_factor > 0.f && backoff_factor < 1.f && growth_interval > 0,
                 "mudg_loss_scale_update: bad arguments");
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, hs(stream), reinterpret_cast<ScaleRecord*>(record), growth_factor,
                       backoff_factor, growth_interval);
    return mudg_check_launch("mudg_loss_scale_update");
}

}  // extern "C"
