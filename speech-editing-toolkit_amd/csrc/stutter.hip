// StutterSpeech's classification head with its two losses, fused (modules/speech_editing/stutter_speech/stutter_predictor.py:15-65,
// tasks/speech_editing/stutter_speech.py:97-99):
//   logits[b][t][j] = bias[j] + sum_c W[j][c] h[b][c][t]                       (nn.Linear(H, 3) on the post_net1 output)
//   ce    = mean over rows with label != 2 of -log p_y                         (nn.CrossEntropyLoss(ignore_index=2))
//   focal = mean over ALL B*T rows of -alpha_y (1 - p_y - s)^3 (log p_y + s)   (MultiFocalLoss, s = 1e-6, alpha = {5e-3, 1, 0})
// log p_y = (z_y - max z) - log(sum exp(z - max z)): finite where the reference's log(softmax) underflows to log(0), and blind to an offset
// common to the three logits (z_y - (max z + log sum) rounds at ulp(max z)).  A batch of pad rows alone (no label != 2) gives ce = 0 / 0 =
// NaN as torch does, a finite focal term, and every gradient exactly 0.  Labels outside {0, 1, 2} are clamped to 0 and 2.  Losses are
// per-block partial sums combined in block order by a second launch; weight / bias gradients are per-(utterance, 256-frame chunk) partial
// rows combined in row order.
// Nothing is atomic and nothing is read back to the host: two runs are bit-identical.
#include "common.h"

namespace {

constexpr float kSmooth = 1e-6f;

__device__ __forceinline__ float alpha_of(int y) { return y == 0 ? 5e-3f : (y == 1 ? 1.0f : 0.0f); }
__device__ __forceinline__ int label_of(const int64_t *labels, int64_t i) {
    const int64_t y = labels[i];
    return y < 0 ? 0 : (y > 2 ? 2 : (int)y);  // the host remaps to {0, 1, 2}; clamped for memory safety only
}

// softmax pieces of one row: p[3], log p_y
__device__ __forceinline__ void row_softmax(const float z[3], int y, float p[3], float &logp_y) {
    const float m = fmaxf(fmaxf(z[0], z[1]), z[2]);
    const float e0 = expf(z[0] - m), e1 = expf(z[1] - m), e2 = expf(z[2] - m);
    const float s = (e0 + e1) + e2;
    p[0] = e0 / s; p[1] = e1 / s; p[2] = e2 / s;
    logp_y = (z[y] - m) - logf(s);
}

// block = 4 waves over one utterance's 64-frame tile; lane = frame (coalesced reads along T), wave w takes channels w, w+4, ...
__global__ void __launch_bounds__(256) stutter_head_fwd_kernel(const float *__restrict__ h, const float *__restrict__ w,
                                                               const float *__restrict__ bias, const int64_t *__restrict__ labels,
                                                               float *__restrict__ logits, float *__restrict__ part, int C, int T) {
    __shared__ float red[4][3][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, t = blockIdx.x * 64 + lane;
    const bool tv = t < T;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (tv) {
        const float *hb = h + (int64_t)b * C * T + t;
#pragma unroll 8
        for (int c = wv; c < C; c += 4) {
            const float v = hb[(int64_t)c * T];
            a0 += w[c] * v;
            a1 += w[C + c] * v;
            a2 += w[2 * C + c] * v;
        }
    }
    red[wv][0][lane] = a0;
    red[wv][1][lane] = a1;
    red[wv][2][lane] = a2;
    __syncthreads();
    if (wv != 0) return;
    float z[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) z[j] = (((red[0][j][lane] + red[1][j][lane]) + red[2][j][lane]) + red[3][j][lane]) + bias[j];
    const int64_t row = (int64_t)b * T + t;
    if (tv) {
        logits[row * 3 + 0] = z[0];
        logits[row * 3 + 1] = z[1];
        logits[row * 3 + 2] = z[2];
    }
    if (!labels) return;
    float ce = 0.0f, nv = 0.0f, fo = 0.0f;
    if (tv) {
        const int y = label_of(labels, row);
        float p[3], lp;
        row_softmax(z, y, p, lp);
        if (y != 2) {
            ce = -lp;
            nv = 1.0f;
        }
        const float om = 1.0f - (p[y] + kSmooth);
        fo = -alpha_of(y) * (om * om * om) * (lp + kSmooth);
    }
    ce = wave_sum(ce);
    nv = wave_sum(nv);
    fo = wave_sum(fo);
    if (lane == 0) {
        float *o = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        o[0] = ce;
        o[1] = nv;
        o[2] = fo;
    }
}

// one wave: stats = {ce sum / n_valid, focal sum / (B T), n_valid}; lane l takes partial rows l, l + 64, ... (fixed association)
__global__ void __launch_bounds__(64) stutter_loss_final_kernel(const float *part, int rows, float n_all, float *stats) {
    const int lane = threadIdx.x;
    float ce = 0.0f, nv = 0.0f, fo = 0.0f;
    for (int r = lane; r < rows; r += 64) {
        ce += part[r * 3 + 0];
        nv += part[r * 3 + 1];
        fo += part[r * 3 + 2];
    }
    ce = wave_sum(ce);
    nv = wave_sum(nv);
    fo = wave_sum(fo);
    if (lane == 0) {
        stats[0] = ce / nv;
        stats[1] = fo / n_all;
        stats[2] = nv;
    }
}

constexpr int BWD_CG = 16;   // channels per backward block
constexpr int BWD_TC = 256;  // frames per backward block (one per thread)

// block = (16-channel group, 256-frame chunk, utterance); thread = frame: recompute softmax from the saved logits, write dh for the
// group's channels (coalesced along T) and the weight-gradient partial dz_j h[c][t] of the chunk (one block reduction).
// Partial row r = b * chunks + chunk: part[r][j * C + c] = sum_t dz_j h[b][c][t]; part[r][3 C + j] = sum_t dz_j (channel group 0 only).
__global__ void __launch_bounds__(256) stutter_head_bwd_kernel(const float *__restrict__ h, const float *__restrict__ w,
                                                               const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                               const float *__restrict__ stats, const float *__restrict__ g_ce,
                                                               const float *__restrict__ g_focal, float *__restrict__ dh,
                                                               float *__restrict__ part, int C, int T, float inv_all) {
    __shared__ float red[4][3 * BWD_CG + 3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = blockIdx.x * BWD_CG, b = blockIdx.z;
    const float gce = g_ce ? *g_ce : 0.0f, gfo = g_focal ? *g_focal : 0.0f;
    const float kce = gce / stats[2];
    float acc[3][BWD_CG], accb[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < BWD_CG; ++k) acc[j][k] = 0.0f;
    const float *hb = h + (int64_t)b * C * T;
    float *dhb = dh + (int64_t)b * C * T;
    for (int t = blockIdx.y * BWD_TC + tid; t < T && t < (blockIdx.y + 1) * BWD_TC; t += 256) {
        const int64_t row = (int64_t)b * T + t;
        const int y = label_of(labels, row);
        const float z[3] = {logits[row * 3], logits[row * 3 + 1], logits[row * 3 + 2]};
        float p[3], lp;
        row_softmax(z, y, p, lp);
        const float q = p[y], om = 1.0f - (q + kSmooth), ls = lp + kSmooth;
        const float ay = alpha_of(y) * (om * om * om - 3.0f * q * (om * om) * ls);
        const float k = -(y != 2 ? kce : 0.0f) - gfo * ay * inv_all;
        float dz[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) dz[j] = ((j == y ? 1.0f : 0.0f) - p[j]) * k;
#pragma unroll
        for (int j = 0; j < 3; ++j) accb[j] += dz[j];
#pragma unroll
        for (int kk = 0; kk < BWD_CG; ++kk) {
            const int c = c0 + kk;
            if (c < C) {
                const float v = hb[(int64_t)c * T + t];
                dhb[(int64_t)c * T + t] = (dz[0] * w[c] + dz[1] * w[C + c]) + dz[2] * w[2 * C + c];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[j][kk] += dz[j] * v;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int kk = 0; kk < BWD_CG; ++kk) {
            const float s = wave_sum(acc[j][kk]);
            if (lane == 0) red[wv][j * BWD_CG + kk] = s;
        }
        const float s = wave_sum(accb[j]);
        if (lane == 0) red[wv][3 * BWD_CG + j] = s;
    }
    __syncthreads();
    if (tid < 3 * BWD_CG + 3) {
        const float s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        float *pb = part + ((int64_t)b * gridDim.y + blockIdx.y) * (3 * C + 3);
        if (tid < 3 * BWD_CG) {
            const int j = tid / BWD_CG, c = c0 + tid % BWD_CG;
            if (c < C) pb[j * C + c] = s;
        } else if (blockIdx.x == 0) {
            pb[3 * C + (tid - 3 * BWD_CG)] = s;
        }
    }
}

// dw[j][c] += sum_r part[r][j C + c], db[j] += sum_r part[r][3 C + j]   (row order)
__global__ void __launch_bounds__(256) stutter_head_wgrad_reduce_kernel(const float *__restrict__ part, int B, int C, float *__restrict__ dw,
                                                                        float *__restrict__ db) {
    const int o = blockIdx.x * 256 + threadIdx.x, n = 3 * C + 3;
    if (o >= n) return;
    float s = 0.0f;
#pragma unroll 16
    for (int r = 0; r < B; ++r) s += part[(int64_t)r * n + o];  // loads issued ahead, sum in row order
    if (o < 3 * C) dw[o] += s;
    else db[o - 3 * C] += s;
}

}  // namespace

extern "C" int64_t set_stutter_head_scratch_floats(int32_t B, int32_t C, int32_t T) {
    const int64_t fwd = (int64_t)B * ((T + 63) / 64) * 3, bwd = (int64_t)B * ((T + BWD_TC - 1) / BWD_TC) * (3 * C + 3);
    return fwd > bwd ? fwd : bwd;
}

extern "C" int set_stutter_head_loss(const float *h, const float *w, const float *bias, const int64_t *labels, float *logits, float *stats,
                                     float *scratch, int32_t B, int32_t C, int32_t T, void *stream) {
    SET_REQUIRE(h && w && bias && logits && B > 0 && C > 0 && T > 0 && (!labels || (stats && scratch)), "set_stutter_head_loss");
    const dim3 grid((T + 63) / 64, B);
    hipLaunchKernelGGL(stutter_head_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, h, w, bias, labels, logits, scratch, C, T);
    int rc = set_check_launch("set_stutter_head_loss");
    if (rc || !labels) return rc;
    hipLaunchKernelGGL(stutter_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scratch, (int)(grid.x * grid.y),
                       (float)((int64_t)B * T), stats);
    return set_check_launch("set_stutter_head_loss(final)");
}

extern "C" int set_stutter_head_bwd_reduce(const float *scratch, float *dw, float *db, int32_t B, int32_t C, int32_t T, void *stream) {
    SET_REQUIRE(scratch && dw && db && B > 0 && C > 0 && T > 0, "set_stutter_head_bwd_reduce");
    hipLaunchKernelGGL(stutter_head_wgrad_reduce_kernel, dim3(set_blocks(3 * C + 3, 256)), dim3(256), 0, (hipStream_t)stream, scratch,
                       B * ((T + BWD_TC - 1) / BWD_TC), C, dw, db);
    return set_check_launch("set_stutter_head_bwd_reduce");
}

extern "C" int set_stutter_head_loss_bwd(const float *h, const float *w, const float *logits, const int64_t *labels, const float *stats,
                                         const float *g_ce, const float *g_focal, float *dh, float *dw, float *db, float *scratch,
                                         int32_t B, int32_t C, int32_t T, void *stream) {
    SET_REQUIRE(h && w && logits && labels && stats && dh && scratch && B > 0 && C > 0 && T > 0 && (!dw == !db),
                "set_stutter_head_loss_bwd");
    hipLaunchKernelGGL(stutter_head_bwd_kernel, dim3((C + BWD_CG - 1) / BWD_CG, (T + BWD_TC - 1) / BWD_TC, B), dim3(256), 0, (hipStream_t)stream, h, w, logits, labels,
                       stats, g_ce, g_focal, dh, scratch, C, T, 1.0f / (float)((int64_t)B * T));
    const int rc = set_check_launch("set_stutter_head_loss_bwd");
    if (rc || !dw) return rc;
    return set_stutter_head_bwd_reduce(scratch, dw, db, B, C, T, stream);
}
