// The small elementwise ops of the diffusion model for gfx950, one kernel and one entry point each: the unfused gate and residual / skip
// update of a DiffNet layer (any residual_channels; also the device-side cross-check of the fused kernels), the sinusoidal step embedding,
// Philox normal noise, the posterior step, q_sample, and the self test of the MFMA fragment layout.
#include "common.h"
#include "philox.h"

namespace {
__global__ void __launch_bounds__(256) gate_kernel(const float *y, float *z, int B, int C, int T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * C * T) return;
    const int64_t ct = i % ((int64_t)C * T);
    const int64_t b = i / ((int64_t)C * T);
    const float *yb = y + b * 2 * C * T;
    z[i] = dev_sigmoid(yb[ct]) * tanhf(yb[(int64_t)C * T + ct]);
}
__global__ void __launch_bounds__(256) res_skip_kernel(const float *x_in, const float *o, float *x_out, float *skip,
                                                       int B, int C, int T, int first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * C * T) return;
    const int64_t ct = i % ((int64_t)C * T);
    const int64_t b = i / ((int64_t)C * T);
    const float *ob = o + b * 2 * C * T;
    x_out[i] = (x_in[i] + ob[ct]) / 1.41421356237309504880f;
    const float s = ob[(int64_t)C * T + ct];
    skip[i] = first ? s : skip[i] + s;
}
__global__ void __launch_bounds__(256) sinusoid_kernel(const float *t, float *out, int dim, int n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)dim * n) return;
    const int j = (int)(i / n), k = (int)(i % n);
    const int half = dim / 2;
    const int jj = j < half ? j : j - half;
    // emb = exp(arange(half) * -(ln(1e4)/(half-1)))   (diffnet.py:42-43, all fp32 tensor ops)
    const float e = (float)(9.210340371976184 / (double)(half - 1));  // python float -> fp32 scalar
    const float freq = expf((float)jj * -e);
    const float ang = t[k] * freq;
    out[i] = j < half ? sinf(ang) : cosf(ang);
}

// (Philox4x32-10 + Box-Muller: csrc/philox.h, shared with the step-boundary kernels of csrc/boundary.hip)

// seed_delta (set_rng_seed_delta, may be NULL): a device word ADDED to the seed argument -- a captured graph carries the seed of the
// step it was captured at; the replay of step k stores (seed_k - seed_captured) there and draws exactly the eager step's numbers
__global__ void __launch_bounds__(256) randn_kernel(float *out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t *seed_delta) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;  // quad index
    if (q * 4 >= n) return;
    if (seed_delta) seed += *seed_delta;
    float z[4];
    randn4(seed, offset + (uint64_t)q, z);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (q * 4 + k < n) out[q * 4 + k] = z[k];
}

// x_prev = c1*x0 + c2*x_t + nonzero*exp(0.5*logvar)*eps      (spec_denoiser.py:86-101)
__global__ void __launch_bounds__(256) posterior_kernel(const float *x0, const float *x_t, const float *eps,
                                                        const float *coef4, int64_t coef_bs, float *x_prev,
                                                        int64_t per_batch, int64_t n, uint64_t seed,
                                                        uint64_t offset, const uint64_t *seed_delta) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q * 4 >= n) return;
    if (seed_delta) seed += *seed_delta;
    float z[4];
    if (!eps) randn4(seed, offset + (uint64_t)q, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = q * 4 + k;
        if (i >= n) break;
        const float *cf = coef4 + (i / per_batch) * coef_bs;
        const float mean = cf[0] * x0[i] + cf[1] * x_t[i];
        const float e = eps ? eps[i] : z[k];
        x_prev[i] = mean + cf[3] * expf(0.5f * cf[2]) * e;
    }
}

__global__ void __launch_bounds__(256) q_sample_kernel(const float *x_start, const float *eps, const float *ab2,
                                                       const float *nonpad, float *x_t, int B, int M, int T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * M * T) return;
    const int t = (int)(i % T);
    const int b = (int)(i / ((int64_t)M * T));
    float v = ab2[2 * b] * x_start[i] + ab2[2 * b + 1] * eps[i];
    if (nonpad) v *= nonpad[(int64_t)b * T + t];
    x_t[i] = v;
}

// ---- MFMA layout self test ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) selftest_mfma_kernel(float *max_err) {
    constexpr int K = 8;
    const int lane = threadIdx.x;
    auto Af = [](int i, int k) { return 0.25f * (float)((i * 7 + k * 3) % 11) - 1.0f; };
    auto Bf = [](int k, int j) { return 0.125f * (float)((k * 5 + j * 13) % 17) - 0.75f; };
    f32x16 acc = {0};
    for (int k0 = 0; k0 < K; k0 += 2) {
        const int k = k0 + (lane >> 5);
        acc = mfma32(Af(lane & 31, k), Bf(k, lane & 31), acc);
    }
    float err = 0.0f;
    for (int r = 0; r < 16; ++r) {
        const int row = mfma32_row(r, lane), col = lane & 31;
        float ref = 0.0f;
        for (int k = 0; k < K; ++k) ref = fmaf(Af(row, k), Bf(k, col), ref);
        err = fmaxf(err, fabsf(ref - acc[r]));
    }
    for (int off = 32; off > 0; off >>= 1) err = fmaxf(err, __shfl_xor(err, off));
    if (lane == 0) *max_err = err;
}
}  // namespace

extern "C" int set_gate(const float *y, float *z, int32_t B, int32_t C, int32_t T, void *stream) {
    SET_REQUIRE(y && z && B > 0 && C > 0 && T > 0, "set_gate");
    hipLaunchKernelGGL(gate_kernel, dim3(set_blocks((int64_t)B * C * T, 256)), dim3(256), 0, (hipStream_t)stream, y, z,
                       B, C, T);
    return set_check_launch("set_gate");
}
extern "C" int set_res_skip(const float *x_in, const float *o, float *x_out, float *skip, int32_t B, int32_t C,
                            int32_t T, int32_t first, void *stream) {
    SET_REQUIRE(x_in && o && x_out && skip && B > 0 && C > 0 && T > 0, "set_res_skip");
    hipLaunchKernelGGL(res_skip_kernel, dim3(set_blocks((int64_t)B * C * T, 256)), dim3(256), 0, (hipStream_t)stream,
                       x_in, o, x_out, skip, B, C, T, first);
    return set_check_launch("set_res_skip");
}
extern "C" int set_sinusoid_embed(const float *t, float *out, int32_t dim, int32_t n, void *stream) {
    SET_REQUIRE(t && out && dim >= 4 && (dim % 2) == 0 && n > 0, "set_sinusoid_embed");
    hipLaunchKernelGGL(sinusoid_kernel, dim3(set_blocks((int64_t)dim * n, 256)), dim3(256), 0, (hipStream_t)stream, t,
                       out, dim, n);
    return set_check_launch("set_sinusoid_embed");
}
static const uint64_t *g_seed_delta = nullptr;
const uint64_t *set_seed_delta_ptr() { return g_seed_delta; }
extern "C" int set_rng_seed_delta(const uint64_t *dev_word) {
    g_seed_delta = dev_word;
    return SET_OK;
}

extern "C" int set_randn(float *out, int64_t n, uint64_t seed, uint64_t offset, void *stream) {
    SET_REQUIRE(out && n > 0, "set_randn");
    hipLaunchKernelGGL(randn_kernel, dim3(set_blocks((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, out, n,
                       seed, offset, g_seed_delta);
    return set_check_launch("set_randn");
}
extern "C" int set_posterior_step(const float *x0, const float *x_t, const float *eps, const float *coef4,
                                  int64_t coef_bs, float *x_prev, int32_t B, int64_t per_batch, uint64_t seed,
                                  uint64_t offset, void *stream) {
    SET_REQUIRE(x0 && x_t && coef4 && x_prev && B > 0 && per_batch > 0, "set_posterior_step");
    const int64_t n = (int64_t)B * per_batch;
    hipLaunchKernelGGL(posterior_kernel, dim3(set_blocks((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, x0,
                       x_t, eps, coef4, coef_bs, x_prev, per_batch, n, seed, offset, g_seed_delta);
    return set_check_launch("set_posterior_step");
}
extern "C" int set_q_sample(const float *x_start, const float *eps, const float *ab2, const float *nonpad, float *x_t,
                            int32_t B, int32_t M, int32_t T, void *stream) {
    SET_REQUIRE(x_start && eps && ab2 && x_t && B > 0 && M > 0 && T > 0, "set_q_sample");
    hipLaunchKernelGGL(q_sample_kernel, dim3(set_blocks((int64_t)B * M * T, 256)), dim3(256), 0, (hipStream_t)stream,
                       x_start, eps, ab2, nonpad, x_t, B, M, T);
    return set_check_launch("set_q_sample");
}
extern "C" int set_selftest_mfma(float *max_err_host, void *stream) {
    SET_REQUIRE(max_err_host != nullptr, "set_selftest_mfma");
    float *d = nullptr;
    SET_HIP(hipMalloc(&d, sizeof(float)), "set_selftest_mfma");
    hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d);
    int rc = set_check_launch("set_selftest_mfma");
    if (rc == SET_OK) {
        hipError_t e = hipMemcpyAsync(max_err_host, d, sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) rc = set_fail(SET_E_LAUNCH, "set_selftest_mfma", hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}
