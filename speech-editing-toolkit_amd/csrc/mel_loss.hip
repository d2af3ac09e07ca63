// HiFi-GAN mel loss, mean |ln mel(y_hat) - ln mel(y)| (tasks/vocoder/hifigan.py:35-38 on modules/vocoder/hifigan/mel_utils.py:59-76), and
// its gradient with respect to the generated waveform.  n_fft = 1024, hop = 256.  Launches:
//   set_mel_linear    log_mel_kernel<LinearMelPolicy> of dft_gemm.h: the filterbank product itself (finish = identity), for y and for y_hat.
//   set_mel_loss_fwd  mel_loss_elem_kernel: both logs (double, rounded once: LogMelPolicy::finish), |dL| summed per block in a fixed
//                     order, g_mel = sign(dL) [mel_hat >= floor] / mel_hat -- count times the loss's gradient: the factor 1 / count is
//                     applied once, at the very end, so that a row's gradient has the same bits before it whatever the batch;
//                     mel_loss_sum_kernel: the blocks' partials (rows_sum.h).
//   set_mel_loss_bwd  mel_spec_bwd_kernel: per 64-frame tile re / im of y_hat again (GEMM 1 of dft_gemm.h: same table image, same LDS
//                       slice), g_mag = basis^T g_mel on the MFMA with re / im's own register layout, g_re = g_mag re / mag, g_im likewise,
//                       to the scratch spec [B][2][32 chunks][Ts].
//                     mel_idft_kernel: the transposed "K = 4 taps, Cin = 256" view, g_p[256 u + c] = sum_q sum_f W[.][f][256 q + c]
//                       g[.][f][u - q], as a gather: a block owns 64 hops x 256 samples of the padded gradient, nobody else writes them.
//                     mel_fold_kernel: reflect fold onto the row, the division by count, the input clamp's mask.  Every sample of g_wav
//                       is written.
// No atomics anywhere; every sum has one fixed order.
#include "dft_gemm.h"  // log_mel_kernel<P>, dft_stage_slice, dft_chunk_spectrum
#include "rows_sum.h"

namespace {

struct LinearMelPolicy {
    static constexpr int MB = 3;
    static __device__ __forceinline__ int frames(int len, int pad) { return len + 2 * pad >= MEL_NFFT ? 1 + (len + 2 * pad - MEL_NFFT) / MEL_HOP : 0; }
    static __device__ __forceinline__ float magnitude(float re, float im, const SetLogMelArgs &a) { return sqrtf((re * re + im * im) + a.mag_eps); }
    static __device__ __forceinline__ float finish(float v, const SetLogMelArgs &) { return v; }
};

// ---- loss and mel gradient ---------------------------------------------------------------------------------------------------------
constexpr int ML_PER_THREAD = 16, ML_PER_BLOCK = 256 * ML_PER_THREAD;

// Block k takes elements [4096 k, 4096 k + 4096); thread tid the elements 4096 k + 256 i + tid, i = 0..15, summed in ascending i.  Column
// tl = tid & 63 of the block = ((s[tl] + s[64 + tl]) + s[128 + tl]) + s[192 + tl] -> part[k][tl].
__global__ void __launch_bounds__(256) mel_loss_elem_kernel(SetMelLossFwdArgs a, int64_t n, float gscale) {
    __shared__ float red[4][64];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * ML_PER_BLOCK + tid;
    float s = 0.0f;
#pragma unroll 4
    for (int i = 0; i < ML_PER_THREAD; ++i) {
        const int64_t e = base + (int64_t)i * 256;
        if (e < n) {
            const float mh = a.mel_hat[e], my = a.mel_y[e];
            const float lh = (float)(a.log_scale * log((double)fmaxf(mh, a.floor)));
            const float ly = (float)(a.log_scale * log((double)fmaxf(my, a.floor)));
            const float d = lh - ly;
            s += fabsf(d);
            a.g_mel[e] = (mh >= a.floor && d != 0.0f) ? copysignf(gscale, d) / mh : 0.0f;
            if (a.log_hat) a.log_hat[e] = lh;
            if (a.log_y) a.log_y[e] = ly;
        }
    }
    red[tid >> 6][tid & 63] = s;
    __syncthreads();
    if (tid < 64) a.part[(int64_t)blockIdx.x * 64 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// loss = (sum of part [rows][64]) / count: the columns by rows_sum.h, then the 64 column sums in ascending order; the division in double
__global__ void __launch_bounds__(1024) mel_loss_sum_kernel(const float *__restrict__ part, int rows, double count, float *__restrict__ loss) {
    __shared__ float red[ROWS_RG][64];
    __shared__ float col[64];
    const int tl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const float t = rows_sum_groups(rows_sum_chains(part + tl, 64, rg, rows), red, rg, tl);
    if (rg == 0) col[tl] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        for (int c = 0; c < 64; ++c) tot += col[c];
        loss[0] = (float)((double)tot / count);
    }
}

// ---- spectral backward ---------------------------------------------------------------------------------------------------------------
constexpr int MEL_KSTEPS_T = 48;  // k-steps (two mel rows each) of the transposed filterbank image: 96 rows

__global__ void __launch_bounds__(256, 2) mel_spec_bwd_kernel(SetMelLossBwdArgs a, int nchunks, int Ts) {
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * MEL_TT;
    dft_stage_slice(S, a.wav + (int64_t)b * a.wav_bs, a.N, t0, a.pad, 1, 1, tid);
    __syncthreads();
    const int h = lane >> 5, j = lane & 31;
    // the two frames of this lane (column blocks 0 and 1); beyond T the mel gradient reads as 0 and so does everything after it
    const bool live0 = t0 + j < a.T, live1 = t0 + 32 + j < a.T;
    const float *__restrict__ g0 = a.g_mel + ((int64_t)b * a.T + (live0 ? t0 + j : 0)) * a.n_mels;
    const float *__restrict__ g1 = a.g_mel + ((int64_t)b * a.T + (live1 ? t0 + 32 + j : 0)) * a.n_mels;
    const int ksteps = (a.n_mels + 1) / 2;
    // one chunk per wave: blockIdx.z takes chunks 4 z .. 4 z + 3.  A chunk's work and output are its own (no sum crosses chunks here), so
    // the split changes no bit; it trades a re-staged slice (68 KB of L2 reads against 2,048 MFMAs per wave) for three times the blocks,
    // which is what a training segment's handful of tiles needs to reach every CU.
    for (int ch = blockIdx.z * 4 + wv; ch < nchunks; ch += 4 * gridDim.z) {
        f32x16 re[2], im[2], gm[2];
        dft_chunk_spectrum(a.table, ch, S, lane, re, im);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) gm[cb][r] = 0.0f;
        // g_mag[bin][t] = sum_m basis[m][bin] g_mel[t][m].  Image: [chunk][k-step s][lane] = basis[2 s + (lane >> 5)][bin_lo + 32 chunk + (lane & 31)]
        const float *__restrict__ bt = a.basis_t + (int64_t)ch * MEL_KSTEPS_T * 64 + lane;
        for (int s0 = 0; s0 < ksteps; s0 += 8) {
            float A[8], B0[8], B1[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int m = 2 * (s0 + u) + h;
                const bool in = m < a.n_mels;
                A[u] = bt[(s0 + u) * 64];
                B0[u] = g0[in ? m : 0];
                B1[u] = g1[in ? m : 0];
                B0[u] = in && live0 ? B0[u] : 0.0f;
                B1[u] = in && live1 ? B1[u] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                gm[0] = mfma32(A[u], B0[u], gm[0]);
                gm[1] = mfma32(A[u], B1[u], gm[1]);
            }
        }
        // g_re = g_mag re / mag, g_im = g_mag im / mag (mag >= sqrt(mag_eps) > 0); spec [b][part][32 ch + bin row][Ts], frames along a row
        float *__restrict__ o = a.spec + ((int64_t)b * 2 * nchunks * 32 + ch * 32 + 4 * h) * Ts + t0 + j;
        const int64_t part = (int64_t)nchunks * 32 * Ts;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float x = re[cb][r], y = im[cb][r];
                const float q = gm[cb][r] / sqrtf((x * x + y * y) + a.mag_eps);
                const int64_t at = (int64_t)urow16(r) * Ts + 32 * cb;
                o[at] = q * x;
                o[part + at] = q * y;
            }
    }
}

// ---- inverse DFT as a matrix product, overlap-add as a gather -------------------------------------------------------------------------
constexpr int ID_U = MEL_TT + 3;           // frames a 64-hop tile gathers from: u0 - 3 .. u0 + 63
constexpr int ID_ROWS = 64;                // rows of a staged slab: 2 parts x 32 bins
constexpr int ID_PER_THREAD = (ID_ROWS * ID_U + 255) / 256;  // 17

// Block = 64 hops x all 256 samples of a hop, of one row; wave w owns samples 64 w .. 64 w + 63 (two 32-row blocks) of both 32-hop column
// blocks.  K runs over (chunk, tap q, part, bin): per chunk the slab G[part][bin][frame] is staged once and read at frame offset 3 - q.
// Image: [chunk][wave][q][part][k-step s][lane][2] = W[part][32 chunk + 2 s + (lane >> 5)][256 q + 64 wave + 32 e + (lane & 31)], e = 0, 1.
__global__ void __launch_bounds__(256, 2) mel_idft_kernel(SetMelLossBwdArgs a, int nchunks, int Ts) {
    __shared__ float G[ID_ROWS * ID_U];
    typedef AVec<2>::type a2_t;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, u0 = blockIdx.x * MEL_TT;
    const int h = lane >> 5, j = lane & 31;
    const float *__restrict__ spec = a.spec + (int64_t)b * 2 * nchunks * 32 * Ts;
    const int64_t part = (int64_t)nchunks * 32 * Ts;
    float st[ID_PER_THREAD];
    auto fetch = [&](int ch) {
#pragma unroll
        for (int k = 0; k < ID_PER_THREAD; ++k) {
            const int idx = tid + 256 * k, row = idx / ID_U, t = u0 - 3 + (idx - row * ID_U);
            const bool in = row < ID_ROWS && t >= 0 && t < Ts;
            const float v = spec[in ? (int64_t)(row >> 5) * part + (int64_t)(ch * 32 + (row & 31)) * Ts + t : 0];
            st[k] = in ? v : 0.0f;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][cb][r] = 0.0f;
    fetch(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        __syncthreads();  // the previous chunk's reads of the slab are done
#pragma unroll
        for (int k = 0; k < ID_PER_THREAD; ++k)
            if (tid + 256 * k < ID_ROWS * ID_U) G[tid + 256 * k] = st[k];
        __syncthreads();
        if (ch + 1 < nchunks) fetch(ch + 1);  // in flight under this chunk's MFMAs
        const a2_t *wp = reinterpret_cast<const a2_t *>(a.itable) + ((int64_t)(ch * 4 + wv) * 128) * 64 + lane;
        // group g of 8 k-steps: k-step kk = 8 g .. 8 g + 7, q = kk >> 5, part = (kk >> 4) & 1, bin pair s = kk & 15
        auto slab = [&](int g) { return G + (((g >> 1) & 1) * 32 + 16 * (g & 1) + h) * ID_U + j + 3 - (g >> 2); };
        const float *bp = slab(0);
        gemm_groups<2, 2, 8>(acc, wp, bp, 2 * ID_U, 16, [&](int g) {
            wp += 8 * 64;
            bp = slab(g + 1);
        });
    }
    // registers 4 g .. 4 g + 3 of a lane are four consecutive samples of its hop: one 16-byte store
    const int U = a.T + 3;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int u = u0 + 32 * cb + j;
        if (u >= U) continue;
        float *__restrict__ o = a.g_pad + ((int64_t)b * U + u) * MEL_HOP + 64 * wv + 4 * h;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[rb][cb][4 * g + e];
                *reinterpret_cast<f32x4 *>(o + 32 * rb + 8 * g) = v;
            }
    }
}

// g_wav[j] = [-1 <= y_hat[j] <= 1] ((g_p[j + P] + mirror about sample 0) + mirror about sample N - 1) / count; g_p reads as 0 at and beyond
// its (T + 3) hop samples (no frame covers those)
__global__ void __launch_bounds__(256) mel_fold_kernel(SetMelLossBwdArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= a.N) return;
    const int64_t Lp = (int64_t)(a.T + 3) * MEL_HOP;
    const float *__restrict__ gp = a.g_pad + (int64_t)b * Lp;
    const int P = a.pad;
    auto at = [&](int64_t i) { return i < Lp ? gp[i] : 0.0f; };
    float v = at((int64_t)j + P);
    if (j >= 1 && j <= P) v += at(P - j);
    if (j >= a.N - 1 - P && j <= a.N - 2) v += at((int64_t)P + 2 * ((int64_t)a.N - 1) - j);
    const float x = a.wav[(int64_t)b * a.wav_bs + j];
    a.g_wav[(int64_t)b * a.N + j] = (x >= -1.0f && x <= 1.0f) ? v / a.count : 0.0f;
}

}  // namespace

extern "C" int64_t set_sizeof_mel_loss_fwd_args(void) { return (int64_t)sizeof(SetMelLossFwdArgs); }
extern "C" int64_t set_sizeof_mel_loss_bwd_args(void) { return (int64_t)sizeof(SetMelLossBwdArgs); }

extern "C" int set_mel_linear(const SetLogMelArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_mel_linear");
    const SetLogMelArgs &a = *args;
    SET_REQUIRE(a.wav && a.table && a.basis && a.mel, "set_mel_linear");
    SET_REQUIRE(a.B > 0 && a.N > 0 && a.T > 0 && a.wav_bs >= a.N && a.n_fft > 0 && a.hop > 0 && a.n_mels > 0, "set_mel_linear");
    if (a.n_fft != MEL_NFFT || a.hop != MEL_HOP || a.n_mels > 32 * LinearMelPolicy::MB)
        return set_fail(SET_E_UNSUPPORTED, "set_mel_linear", "built for n_fft = 1024, hop = 256, n_mels <= 96");
    SET_REQUIRE(a.bin_lo >= 0 && a.bin_lo % 32 == 0 && a.nbins > 0 && a.bin_lo + a.nbins <= MEL_NBIN_ALL, "set_mel_linear");
    SET_REQUIRE(a.pad >= 0 && a.pad <= MEL_NFFT / 2 && (a.reflect == 0 || a.reflect == 1) && (a.clamp_input == 0 || a.clamp_input == 1),
                "set_mel_linear");
    SET_REQUIRE(!a.reflect || a.N > a.pad, "set_mel_linear");
    SET_REQUIRE((int64_t)a.N + 2 * a.pad >= MEL_NFFT && a.T == 1 + (a.N + 2 * a.pad - MEL_NFFT) / MEL_HOP, "set_mel_linear");
    SET_REQUIRE(a.mag_eps >= 0.0f, "set_mel_linear");
    SET_REQUIRE((int64_t)a.B * a.T * a.n_mels < (int64_t)1 << 40 && a.B <= 65535, "set_mel_linear");
    SET_REQUIRE(set_aligned16(a.table, a.basis, (a.n_mels & 3) == 0 ? (const void *)a.mel : nullptr), "set_mel_linear");
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, MEL_LDS, "set_mel_linear attr", log_mel_kernel<LinearMelPolicy>)) return rc;
    const dim3 grid((a.T + MEL_TT - 1) / MEL_TT, a.B);
    hipLaunchKernelGGL(log_mel_kernel<LinearMelPolicy>, grid, dim3(256), MEL_LDS, (hipStream_t)stream, a, (a.nbins + 31) / 32);
    return set_check_launch("set_mel_linear");
}

extern "C" int64_t set_mel_loss_fwd_scratch_floats(int64_t count) { return count > 0 ? (count + ML_PER_BLOCK - 1) / ML_PER_BLOCK * 64 : 0; }

extern "C" int set_mel_loss_fwd(const SetMelLossFwdArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_mel_loss_fwd");
    const SetMelLossFwdArgs &a = *args;
    SET_REQUIRE(a.mel_hat && a.mel_y && a.g_mel && a.part && a.loss, "set_mel_loss_fwd");
    SET_REQUIRE(a.B > 0 && a.T > 0 && a.n_mels > 0 && a.floor > 0.0f && a.log_scale > 0.0, "set_mel_loss_fwd");
    const int64_t n = (int64_t)a.B * a.T * a.n_mels;
    SET_REQUIRE(n < (int64_t)1 << 40, "set_mel_loss_fwd");
    const int64_t blocks = (n + ML_PER_BLOCK - 1) / ML_PER_BLOCK;
    SET_REQUIRE(blocks < (int64_t)1 << 30, "set_mel_loss_fwd");
    hipLaunchKernelGGL(mel_loss_elem_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, n, (float)a.log_scale);
    if (int rc = set_check_launch("set_mel_loss_fwd")) return rc;
    hipLaunchKernelGGL(mel_loss_sum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a.part, (int)blocks, (double)n, a.loss);
    return set_check_launch("set_mel_loss_fwd sum");
}

extern "C" int64_t set_mel_idft_table_size(int32_t n_fft, int32_t nbins) {
    if (n_fft <= 0 || nbins <= 0) return 0;
    return 2 * (int64_t)((nbins + 31) / 32 * 32) * n_fft;
}
extern "C" int64_t set_mel_loss_bwd_spec_floats(int32_t B, int32_t T, int32_t nbins) {
    if (B <= 0 || T <= 0 || nbins <= 0) return 0;
    return (int64_t)B * 2 * ((nbins + 31) / 32 * 32) * ((T + MEL_TT - 1) / MEL_TT * MEL_TT);
}

extern "C" int set_mel_loss_bwd(const SetMelLossBwdArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_mel_loss_bwd");
    const SetMelLossBwdArgs &a = *args;
    SET_REQUIRE(a.wav && a.table && a.basis_t && a.itable && a.g_mel && a.spec && a.g_pad && a.g_wav, "set_mel_loss_bwd");
    SET_REQUIRE(a.B > 0 && a.N > 0 && a.T > 0 && a.wav_bs >= a.N && a.n_fft > 0 && a.hop > 0 && a.n_mels > 0, "set_mel_loss_bwd");
    if (a.n_fft != MEL_NFFT || a.hop != MEL_HOP || a.n_mels > 2 * MEL_KSTEPS_T)
        return set_fail(SET_E_UNSUPPORTED, "set_mel_loss_bwd", "built for n_fft = 1024, hop = 256, n_mels <= 96");
    if (a.pad != (MEL_NFFT - MEL_HOP) / 2)
        return set_fail(SET_E_UNSUPPORTED, "set_mel_loss_bwd", "built for the reflect padding of (n_fft - hop) / 2 with the input clamp");
    SET_REQUIRE(a.bin_lo >= 0 && a.bin_lo % 32 == 0 && a.nbins > 0 && a.bin_lo + a.nbins <= MEL_NBIN_ALL, "set_mel_loss_bwd");
    SET_REQUIRE(a.N > a.pad, "set_mel_loss_bwd");  // torch's reflect pad refuses pad >= length too
    SET_REQUIRE((int64_t)a.N + 2 * a.pad >= MEL_NFFT && a.T == 1 + (a.N + 2 * a.pad - MEL_NFFT) / MEL_HOP, "set_mel_loss_bwd");
    SET_REQUIRE(a.mag_eps > 0.0f && a.count > 0.0f, "set_mel_loss_bwd");  // both are divided by
    SET_REQUIRE(a.B <= 65535 && (int64_t)a.N + 2 * a.pad < (int64_t)1 << 30, "set_mel_loss_bwd");
    SET_REQUIRE(set_aligned16(a.table, a.itable, a.g_pad), "set_mel_loss_bwd");
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, MEL_LDS, "set_mel_loss_bwd attr", mel_spec_bwd_kernel)) return rc;
    const int nchunks = (a.nbins + 31) / 32, tiles = (a.T + MEL_TT - 1) / MEL_TT, Ts = tiles * MEL_TT;
    hipLaunchKernelGGL(mel_spec_bwd_kernel, dim3(tiles, a.B, (nchunks + 3) / 4), dim3(256), MEL_LDS, (hipStream_t)stream, a, nchunks, Ts);
    if (int rc = set_check_launch("set_mel_loss_bwd spectrum")) return rc;
    hipLaunchKernelGGL(mel_idft_kernel, dim3((a.T + 3 + MEL_TT - 1) / MEL_TT, a.B), dim3(256), 0, (hipStream_t)stream, a, nchunks, Ts);
    if (int rc = set_check_launch("set_mel_loss_bwd inverse")) return rc;
    hipLaunchKernelGGL(mel_fold_kernel, dim3((a.N + 255) / 256, a.B), dim3(256), 0, (hipStream_t)stream, a);
    return set_check_launch("set_mel_loss_bwd fold");
}
