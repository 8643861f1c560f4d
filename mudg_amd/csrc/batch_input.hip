// batch_input.hip — the two elementwise kernels of LatentVisualDiffusion.get_batch_input (reference ddpm3d.py:1064-1149): the
// posterior sample of the three VAE encodes written straight into z / c_concat, and the conditioning dropout of the prompt
// rows and the key-frame image from the device-side uniform draw.  fp32 in, fp32 out; no operand type.
#include "common.h"

namespace {

// One value of DiagonalGaussianDistribution.sample: the statements of gaussian_sample_kernel (misc.hip), which this kernel must
// reproduce bit for bit (-ffp-contract=off: the multiply and the add stay separate here as there).
__device__ __forceinline__ float posterior_value(float mean, float lv, float noise, bool has_noise, float scale) {
    lv = fminf(fmaxf(lv, -30.f), 20.f);
    float z = mean;
    if (has_noise) z = mean + expf(0.5f * lv) * noise;
    return scale * z;
}

struct Streams {
    const float* mom[3];     // dense, sparse colour, sparse depth: (N, 2C, HW)
    const float* noise[3];   // (N, C, HW) each, or all NULL (posterior mode)
};

// V = 4: 16-byte accesses along HW (HW % 4 == 0, every base 16-byte aligned); V = 1: any shape.
// Work item = V consecutive positions of (stream, frame n = b T + t, channel c).
template <int V>
__global__ __launch_bounds__(256) void posterior_assemble_kernel(Streams s, float* __restrict__ z, float* __restrict__ cc, int T, int C,
                                                                 int64_t HW, float scale, int64_t per_stream, int64_t total) {
    const int64_t hwv = HW / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int st = (int)(i / per_stream);
        int64_t r = i - st * per_stream;
        const int64_t p = (r % hwv) * V;
        r /= hwv;
        const int c = (int)(r % C);
        const int64_t n = r / C;
        const int64_t b = n / T, t = n - b * T;
        // (selected, not indexed: a run-time index into the by-value argument struct would put it into scratch)
        const float* mom0 = st == 0 ? s.mom[0] : st == 1 ? s.mom[1] : s.mom[2];
        const float* nz0 = st == 0 ? s.noise[0] : st == 1 ? s.noise[1] : s.noise[2];
        const float* mom = mom0 + (n * 2 * C + c) * HW + p;
        const float* nz = nz0 ? nz0 + (n * C + c) * HW + p : nullptr;
        // z: (B, C, T, HW); c_concat: (B, 2C, T, HW) with the sparse colour latents in channels [0, C), sparse depth in [C, 2C)
        float* out = st == 0 ? z + ((b * C + c) * T + t) * HW + p : cc + ((b * 2 * C + (st - 1) * C + c) * T + t) * HW + p;
        if constexpr (V == 4) {
            const float4 m = *reinterpret_cast<const float4*>(mom);
            const float4 l = *reinterpret_cast<const float4*>(mom + (int64_t)C * HW);
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nz) e = *reinterpret_cast<const float4*>(nz);
            float4 o;
            o.x = posterior_value(m.x, l.x, e.x, nz != nullptr, scale);
            o.y = posterior_value(m.y, l.y, e.y, nz != nullptr, scale);
            o.z = posterior_value(m.z, l.z, e.z, nz != nullptr, scale);
            o.w = posterior_value(m.w, l.w, e.w, nz != nullptr, scale);
            *reinterpret_cast<float4*>(out) = o;
        } else {
            out[0] = posterior_value(mom[0], mom[(int64_t)C * HW], nz ? nz[0] : 0.f, nz != nullptr, scale);
        }
    }
}

// Work items [0, B * ld) are the prompt rows, [B * ld, B * ld + B * C * hw) the key-frame image (ld = L D / V, hw = HW / V).
template <int V>
__global__ __launch_bounds__(256) void cond_dropout_kernel(const float* __restrict__ r, float p, float p2, float p3, const float* __restrict__ emb,
                                                           const float* __restrict__ null_prompt, float* __restrict__ prompt_out,
                                                           int64_t LD, const float* __restrict__ img, int64_t img_bstride,
                                                           int64_t img_cstride, float* __restrict__ img_out, int C, int64_t HW,
                                                           int64_t n_prompt, int64_t total) {
    const int64_t ld = LD / V, hw = HW / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (i < n_prompt) {
            const int64_t b = i / ld, k = (i - b * ld) * V;
            const bool drop = r[b] < p2;                                           // prompt_mask (ddpm3d.py:1087)
            const float* src = drop ? null_prompt + k : emb + b * LD + k;
            float* dst = prompt_out + b * LD + k;
            if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
            else dst[0] = src[0];
        } else {
            int64_t j = i - n_prompt;
            const int64_t q = (j % hw) * V;
            j /= hw;
            const int c = (int)(j % C);
            const int64_t b = j / C;
            const float rb = r[b];
            // input_mask = 1 - (r >= p)(r < 3p), multiplied in as the reference does (ddpm3d.py:1088, :1100)
            const float m = 1.f - (rb >= p ? 1.f : 0.f) * (rb < p3 ? 1.f : 0.f);
            const float* src = img + b * img_bstride + c * img_cstride + q;
            float* dst = img_out + (b * C + c) * HW + q;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(src);
                *reinterpret_cast<float4*>(dst) = make_float4(m * x.x, m * x.y, m * x.z, m * x.w);
            } else {
                dst[0] = m * src[0];
            }
        }
    }
}

inline unsigned grid_for(int64_t total) {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks < 4096 ? blocks : 4096);
}

}  // namespace

extern "C" int mudg_posterior_assemble(const float* mom_x, const float* mom_sparse, const float* mom_depth, const float* noise_x,
                                       const float* noise_sparse, const float* noise_depth, float* z, float* c_concat, int B, int T,
                                       int C, int64_t HW, float scale, void* stream) {
    MUDG_REQUIRE(mom_x && mom_sparse && mom_depth && z && c_concat, "mudg_posterior_assemble: null pointer");
    MUDG_REQUIRE(B > 0 && T > 0 && C > 0 && HW > 0, "mudg_posterior_assemble: bad sizes");
    const int have = (noise_x != nullptr) + (noise_sparse != nullptr) + (noise_depth != nullptr);
    MUDG_REQUIRE(have == 0 || have == 3, "mudg_posterior_assemble: noise for all three streams or for none");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    Streams st{{mom_x, mom_sparse, mom_depth}, {noise_x, noise_sparse, noise_depth}};
    bool vec = HW % 4 == 0 && aligned16(z) && aligned16(c_concat);
    for (int i = 0; i < 3; ++i) vec = vec && aligned16(st.mom[i]) && aligned16(st.noise[i]);
    const int slot = mudg_prof_begin(MUDG_FAM_MISC, s);
    const int64_t values = (int64_t)B * T * C * HW;
    if (vec) {
        const int64_t per = values / 4;
        hipLaunchKernelGGL(posterior_assemble_kernel<4>, dim3(grid_for(3 * per)), dim3(256), 0, s, st, z, c_concat, T, C, HW, scale, per, 3 * per);
    } else {
        hipLaunchKernelGGL(posterior_assemble_kernel<1>, dim3(grid_for(3 * values)), dim3(256), 0, s, st, z, c_concat, T, C, HW, scale, values,
                           3 * values);
    }
    const int rc = mudg_check_launch("mudg_posterior_assemble");
    mudg_prof_end(slot, s, 0.0, (double)values * 3.0 * 4.0 * 4.0);
    return rc;
}

extern "C" int mudg_cond_dropout(const float* r, float p, float p2, float p3, const float* cond_emb, const float* null_prompt, float* prompt_out, int B,
                                 int64_t LD, const float* img, int64_t img_bstride, int64_t img_cstride, float* img_out, int C,
                                 int64_t HW, void* stream) {
    MUDG_REQUIRE(r && cond_emb && null_prompt && prompt_out && img && img_out, "mudg_cond_dropout: null pointer");
    MUDG_REQUIRE(B > 0 && LD > 0 && C > 0 && HW > 0, "mudg_cond_dropout: bad sizes");
    MUDG_REQUIRE(img_cstride >= HW && img_bstride >= (int64_t)C * img_cstride, "mudg_cond_dropout: image strides overlap");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool vec = LD % 4 == 0 && HW % 4 == 0 && img_bstride % 4 == 0 && img_cstride % 4 == 0 && aligned16(cond_emb) &&
                     aligned16(null_prompt) && aligned16(prompt_out) && aligned16(img) && aligned16(img_out);
    const int slot = mudg_prof_begin(MUDG_FAM_MISC, s);
    const int v = vec ? 4 : 1;
    const int64_t n_prompt = (int64_t)B * (LD / v), total = n_prompt + (int64_t)B * C * (HW / v);
    if (vec)
        hipLaunchKernelGGL(cond_dropout_kernel<4>, dim3(grid_for(total)), dim3(256), 0, s, r, p, p2, p3, cond_emb, null_prompt, prompt_out, LD, img,
                           img_bstride, img_cstride, img_out, C, HW, n_prompt, total);
    else
        hipLaunchKernelGGL(cond_dropout_kernel<1>, dim3(grid_for(total)), dim3(256), 0, s, r, p, p2, p3, cond_emb, null_prompt, prompt_out, LD, img,
                           img_bstride, img_cstride, img_out, C, HW, n_prompt, total);
    const int rc = mudg_check_launch("mudg_cond_dropout");
    mudg_prof_end(slot, s, 0.0, ((double)B * LD + (double)B * C * HW) * 8.0);
    return rc;
}
