// Multi-resolution STFT loss (modules/vocoder/hifigan/stft_loss.py: spectral convergence ||y_mag - x_mag||_F / ||y_mag||_F and log-magnitude
// mean |log y_mag - log x_mag| of mag = sqrt(clamp(re^2 + im^2, min = 1e-7)), torch.stft centred with reflect padding of n_fft / 2) and its
// gradient with respect to one of the two waveforms.  One resolution per call; the geometry <NFFT, HOP, WIN> is a template parameter and
// STFT_GEOMETRIES lists the instances (a fourth is one line).  Launches:
//   set_stft_magnitude  stft_fwd_kernel<G, 1>: the magnitudes of x to [B][T][NFFT/2 + 1].
//   set_stft_loss_fwd   stft_fwd_kernel<G, 0>: a block = 64 frames x 4 chunks of 32 bins (one per wave) of one row computes the magnitude
//                       tile of x, keeps it in registers, computes that of y, and adds its share of sum (y_mag - x_mag)^2, sum y_mag^2,
//                       sum |log y_mag - log x_mag| in double -> part [block][3]; optionally the magnitudes of the signal that is NOT
//                       differentiated go to a buffer for the backward.  stft_finish_kernel: the blocks' partials in a fixed order ->
//                       the two losses and D, G, count for the backward.
//   set_stft_loss_bwd   stft_spec_bwd_kernel: GEMM 1 again for the differentiated signal (the other's magnitudes from the buffer, or by
//                       a second GEMM 1), g_m from D, G, count and the two upstream scalars (read on the device), g_re = g_m re / m
//                       where re^2 + im^2 >= 1e-7 -> spec [B][2][chunks x 32][Ts];
//                       stft_idft_kernel: the inverse windowed DFT as a gather GEMM, a block owns 64 whole hops of the padded gradient;
//                       stft_fold_kernel: the reflect fold of pad = NFFT / 2 onto the row, written or added to g_wav.
// GEMM 1: A = the table restricted to the WIN non-zero window samples ([chunk][k-step][lane][2] = re, im), B = frames read from the LDS
// image S[c][u] (c = sample within a hop, u = hop, odd row stride) of the padded slice that starts at the window's first sample: frame t,
// window sample HOP q + c is S[c][t + q], lanes read consecutive u (no bank conflict at any hop).  A pipelined body of KB k-steps never
// crosses a hop: KB is chosen per geometry (stft_body).  No atomics anywhere; every sum has one fixed order.
#include "dft_gemm.h"  // padded_index

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

#define STFT_GEOMETRIES(X) X(1024, 120, 600) X(2048, 240, 1200) X(512, 50, 240)

constexpr float STFT_CLAMP = 1e-7f;

// k-steps (2 samples each) of a pipelined body: the largest count up to 12 whose samples divide a hop and whose k-steps divide WIN / 2
constexpr int stft_body(int hop, int win) {
    for (int kb = 12; kb >= 1; --kb)
        if (hop % (2 * kb) == 0 && (win / 2) % kb == 0) return kb;
    return 0;
}

template <int NFFT_, int HOP_, int WIN_>
struct StftGeo {
    static constexpr int NFFT = NFFT_, HOP = HOP_, WIN = WIN_;
    static constexpr int NBIN = NFFT / 2 + 1, NCH = (NBIN + 31) / 32, LEFT = (NFFT - WIN) / 2, PAD = NFFT / 2;
    static constexpr int Q = (WIN + HOP - 1) / HOP;  // hops a window spans
    static constexpr int TT = 64;                    // frames per block
    static constexpr int U = (TT + Q - 1) | 1;       // hops of waveform a tile reads, made odd: the row stride of S
    static constexpr int LDS = HOP * U * 4;
    static constexpr int KB = stft_body(HOP, WIN);
    // the inverse product: one 32-sample row block of a hop per wave, over both 32-hop column blocks (4 or 8 row blocks: 1 or 2 blocks
    // of 4 waves per tile, blockIdx.z), or over one column block (2 row blocks)
    static constexpr int RBT = (HOP + 31) / 32;
    static constexpr int NCB = RBT >= 4 ? 2 : 1, NW = RBT >= 4 ? RBT : 4;  // NW: waves per 64-hop tile
    static constexpr int ID_U = TT + Q - 1;  // frames a 64-hop tile gathers from
    static constexpr int IK = Q * 32;        // k-steps of the inverse product per 32-bin chunk: Q taps x 2 parts x 16 bin pairs
    static_assert(KB > 0 && WIN % 2 == 0 && HOP % 2 == 0 && WIN <= NFFT && HOP <= 256, "geometry");
    static_assert(RBT == 2 || RBT == 4 || RBT == 8, "a hop is 2, 4 or 8 row blocks: blocks of 4 waves share them evenly");
    static_assert((IK / 8) % 2 == 0, "gemm_groups wants an even number of groups");
    static_assert(2 * LDS <= 160 * 1024, "two blocks per CU");
};

// ---- the slice: flat index i of the slice is padded sample t0 HOP + LEFT + i (coalesced reads), stored at S[i % HOP][i / HOP]: consecutive
//      threads are consecutive c, whose rows lie U = 5 (mod 32) banks apart: no conflict
template <class G>
__device__ __forceinline__ void stft_stage_slice(float *S, const float *__restrict__ x, int N, int t0, int tid) {
    const int64_t i0 = (int64_t)t0 * G::HOP + G::LEFT;
    constexpr int TOT = G::HOP * G::U, NB = 8;
    for (int base = tid; base < TOT; base += 256 * NB) {
        int idx[NB];
        float v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) idx[k] = base + 256 * k < TOT ? padded_index(i0 + base + 256 * k, N, G::PAD, 1) : -1;
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = x[idx[k] < 0 ? 0 : idx[k]];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = base + 256 * k, u = i / G::HOP, c = i - u * G::HOP;
            if (i < TOT) S[c * G::U + u] = idx[k] < 0 ? 0.0f : v[k];
        }
    }
}

// re / im [cb] of chunk `ch`: register r of lane l = bin 32 ch + urow16(r) + 4 (l >> 5), frame 32 cb + (l & 31) of the tile.  One accumulator
// per (bin, frame) takes the window samples in ascending order.
template <class G>
__device__ __forceinline__ void stft_chunk_spectrum(const float *__restrict__ table, int ch, const float *S, int lane, f32x16 (&re)[2],
                                                    f32x16 (&im)[2]) {
    constexpr int KB = G::KB, NBODY = G::WIN / 2 / KB;
    const int h = lane >> 5, j = lane & 31;
    const f32x2 *__restrict__ wp = reinterpret_cast<const f32x2 *>(table) + (int64_t)ch * (G::WIN / 2) * 64 + lane;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) re[cb][r] = im[cb][r] = 0.0f;
    f32x2 A[KB], An[KB];
#pragma unroll
    for (int p = 0; p < KB; ++p) A[p] = wp[p * 64];
    int q = 0, c0 = 0;  // the body's first window sample is HOP q + c0
    for (int body = 0; body < NBODY; ++body) {
        const int nb = body + 1 < NBODY ? body + 1 : body;  // last body: re-load itself (in bounds, unused)
#pragma unroll
        for (int p = 0; p < KB; ++p) An[p] = wp[(nb * KB + p) * 64];
        __builtin_amdgcn_sched_barrier(0);
        const float *sp = S + (c0 + h) * G::U + q + j;
        float B0[KB], B1[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            B0[u] = sp[u * 2 * G::U];
            B1[u] = sp[u * 2 * G::U + 32];
        }
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            re[0] = mfma32(A[u][0], B0[u], re[0]);
            im[0] = mfma32(A[u][1], B0[u], im[0]);
            re[1] = mfma32(A[u][0], B1[u], re[1]);
            im[1] = mfma32(A[u][1], B1[u], im[1]);
        }
#pragma unroll
        for (int p = 0; p < KB; ++p) A[p] = An[p];
        c0 += 2 * KB;
        if (c0 == G::HOP) {
            c0 = 0;
            ++q;
        }
    }
}

__device__ __forceinline__ float stft_mag(float re, float im) { return sqrtf(fmaxf(re * re + im * im, STFT_CLAMP)); }
// ln evaluated in double and rounded once (the project's rule for logs whose bits a test restates)
__device__ __forceinline__ float stft_log(float m) { return (float)log((double)m); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// MODE 0: the loss partials (and a.mag when not NULL); MODE 1: the magnitudes of x to a.mag [B][T][NBIN]
template <class G, int MODE>
__global__ void __launch_bounds__(256, 2) stft_fwd_kernel(SetStftLossArgs a, int Ts) {
    extern __shared__ __attribute__((aligned(16))) float S[];
    __shared__ double red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * G::TT, ch = blockIdx.z * 4 + wv;
    const bool active = ch < G::NCH;  // wave-uniform
    const int h = lane >> 5, j = lane & 31;
    f32x16 mx[2], re[2], im[2];
    stft_stage_slice<G>(S, a.x + (int64_t)b * a.x_bs, a.N, t0, tid);
    __syncthreads();
    if (active) {
        stft_chunk_spectrum<G>(a.table, ch, S, lane, re, im);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[cb][r] = stft_mag(re[cb][r], im[cb][r]);
    }
    if constexpr (MODE == 1) {
        if (!active) return;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int t = t0 + 32 * cb + j;
            if (t >= a.T) continue;
            float *__restrict__ o = a.mag + ((int64_t)b * a.T + t) * G::NBIN + 32 * ch + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (32 * ch + 4 * h + urow16(r) < G::NBIN) o[urow16(r)] = mx[cb][r];
        }
    } else {
        __syncthreads();  // every wave is done reading the slice of x
        stft_stage_slice<G>(S, a.y + (int64_t)b * a.y_bs, a.N, t0, tid);
        __syncthreads();
        double sd = 0.0, sg = 0.0, sl = 0.0;
        if (active) {
            stft_chunk_spectrum<G>(a.table, ch, S, lane, re, im);
            float *__restrict__ keep = a.mag ? a.mag + ((int64_t)(b * G::NCH + ch) * 32 + 4 * h) * Ts + t0 + j : nullptr;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float xm = mx[cb][r], ym = stft_mag(re[cb][r], im[cb][r]);
                    const bool live = t0 + 32 * cb + j < a.T && 32 * ch + 4 * h + urow16(r) < G::NBIN;
                    const float d = ym - xm, l = fabsf(stft_log(ym) - stft_log(xm));
                    sd += live ? (double)d * (double)d : 0.0;
                    sg += live ? (double)ym * (double)ym : 0.0;
                    sl += live ? (double)l : 0.0;
                    if (keep) keep[(int64_t)urow16(r) * Ts + 32 * cb] = a.which ? xm : ym;
                }
        }
        sd = wave_sum_f64(sd), sg = wave_sum_f64(sg), sl = wave_sum_f64(sl);
        if (lane == 0) red[wv][0] = sd, red[wv][1] = sg, red[wv][2] = sl;
        __syncthreads();
        if (tid < 3) {
            const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + b) * gridDim.x + blockIdx.x;
            a.part[blk * 3 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        }
    }
}

// thread t sums blocks t, t + 256, ... in ascending order; the 256 thread sums in ascending order
__global__ void __launch_bounds__(256) stft_finish_kernel(const double *__restrict__ part, int64_t nblocks, double count,
                                                          double *__restrict__ stats, float *__restrict__ loss) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t k = tid; k < nblocks; k += 256) {
        s0 += part[k * 3];
        s1 += part[k * 3 + 1];
        s2 += part[k * 3 + 2];
    }
    red[0][tid] = s0, red[1][tid] = s1, red[2][tid] = s2;
    __syncthreads();
    if (tid != 0) return;
    double tot[3];
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += red[i][k];
        tot[i] = t;
    }
    const double D = sqrt(tot[0]), Gn = sqrt(tot[1]);
    stats[0] = D, stats[1] = Gn, stats[2] = count, stats[3] = tot[0], stats[4] = tot[1], stats[5] = tot[2];
    loss[0] = (float)(D / Gn);
    loss[1] = (float)(tot[2] / count);
}

// ---- spectral backward -----------------------------------------------------------------------------------------------------------------
template <class G, bool STORED>
__global__ void __launch_bounds__(256, 2) stft_spec_bwd_kernel(SetStftLossArgs a, int Ts) {
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * G::TT, ch = blockIdx.z * 4 + wv;
    const bool active = ch < G::NCH;
    const int h = lane >> 5, j = lane & 31;
    const float *__restrict__ diff = a.which ? a.y + (int64_t)b * a.y_bs : a.x + (int64_t)b * a.x_bs;
    const float *__restrict__ other = a.which ? a.x + (int64_t)b * a.x_bs : a.y + (int64_t)b * a.y_bs;
    f32x16 rm[2], re[2], im[2];
    if constexpr (STORED) {
        if (active) {
            const float *__restrict__ keep = a.mag + ((int64_t)(b * G::NCH + ch) * 32 + 4 * h) * Ts + t0 + j;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) rm[cb][r] = keep[(int64_t)urow16(r) * Ts + 32 * cb];
        }
    } else {
        stft_stage_slice<G>(S, other, a.N, t0, tid);
        __syncthreads();
        if (active) {
            stft_chunk_spectrum<G>(a.table, ch, S, lane, re, im);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) rm[cb][r] = stft_mag(re[cb][r], im[cb][r]);
        }
        __syncthreads();
    }
    stft_stage_slice<G>(S, diff, a.N, t0, tid);
    __syncthreads();
    if (!active) return;
    stft_chunk_spectrum<G>(a.table, ch, S, lane, re, im);
    // g_m = c1 (m - r) - c2 m + c3 sign(m - r) / m: the coefficients in double from the device scalars, rounded once
    // (a given magnitude gradient a.g_m [B][T][NBIN] replaces it: the stage tests' entry)
    float c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
    if (!a.g_m) {
        const double D = a.stats[0], Gn = a.stats[1], cnt = a.stats[2];
        const double us = (double)a.u_sc[0] * (double)a.scale, um = (double)a.u_mag[0] * (double)a.scale;
        c1 = D > 0.0 ? (float)(us / (D * Gn)) : 0.0f;
        c2 = a.which ? (float)(us * D / (Gn * Gn * Gn)) : 0.0f;
        c3 = (float)(um / cnt);
    }
    float *__restrict__ o = a.spec + ((int64_t)(b * 2 * G::NCH + ch) * 32 + 4 * h) * Ts + t0 + j;
    const int64_t part = (int64_t)G::NCH * 32 * Ts;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float x = re[cb][r], y = im[cb][r], p = x * x + y * y, m = sqrtf(fmaxf(p, STFT_CLAMP)), rr = rm[cb][r];
            const bool live = t0 + 32 * cb + j < a.T && 32 * ch + 4 * h + urow16(r) < G::NBIN && p >= STFT_CLAMP;
            const float sgn = m > rr ? 1.0f : (m < rr ? -1.0f : 0.0f);
            const int t = t0 + 32 * cb + j, bin = 32 * ch + 4 * h + urow16(r);
            const float gm = a.g_m ? a.g_m[t < a.T && bin < G::NBIN ? ((int64_t)b * a.T + t) * G::NBIN + bin : 0]
                                   : (c1 * (m - rr) - c2 * m) + c3 * sgn / m;
            const float qv = live ? gm / m : 0.0f;
            const int64_t at = (int64_t)urow16(r) * Ts + 32 * cb;
            o[at] = qv * x;
            o[part + at] = qv * y;
        }
}

// ---- inverse DFT as a matrix product, overlap-add as a gather --------------------------------------------------------------------------
// g_pad[HOP u + c] = sum_chunk sum_q sum_part sum_f W[part][f][HOP q + c] g[part][f][u - q] (window samples HOP q + c < WIN; g_pad's sample
// i is padded sample LEFT + i).  A tile = 64 hops of one row; wave vw = 4 blockIdx.z + (wave of the block) takes row block vw of a hop
// over both 32-hop column blocks (RBT >= 4), or row block vw >> 1 and column block vw & 1 (RBT = 2).  A sample is one accumulator
// whatever the split: the blocks of a tile only share the staged slab's reads.
template <class G>
__global__ void __launch_bounds__(256, 2) stft_idft_kernel(SetStftLossArgs a, int Ts) {
    constexpr int ID_U = G::ID_U, ROWS = 64, PER_THREAD = (ROWS * ID_U + 255) / 256, RB = 1, NCB = G::NCB;
    __shared__ float Gs[ROWS * ID_U];
    typedef typename AVec<RB>::type av_t;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, u0 = blockIdx.x * G::TT;
    const int h = lane >> 5, j = lane & 31;
    const int vw = 4 * blockIdx.z + wv;
    const int cb0 = NCB == 2 ? 0 : (vw & 1), rb0 = NCB == 2 ? vw : (vw >> 1);
    const float *__restrict__ spec = a.spec + (int64_t)b * 2 * G::NCH * 32 * Ts;
    const int64_t part = (int64_t)G::NCH * 32 * Ts;
    float st[PER_THREAD];
    auto fetch = [&](int ch) {
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int idx = tid + 256 * k, row = idx / ID_U, t = u0 - (G::Q - 1) + (idx - row * ID_U);
            const bool in = row < ROWS && t >= 0 && t < Ts;
            const float v = spec[in ? (int64_t)(row >> 5) * part + (int64_t)(ch * 32 + (row & 31)) * Ts + t : 0];
            st[k] = in ? v : 0.0f;
        }
    };
    f32x16 acc[RB][NCB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][cb][r] = 0.0f;
    fetch(0);
    for (int ch = 0; ch < G::NCH; ++ch) {
        __syncthreads();  // the previous chunk's reads of the slab are done
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k)
            if (tid + 256 * k < ROWS * ID_U) Gs[tid + 256 * k] = st[k];
        __syncthreads();
        if (ch + 1 < G::NCH) fetch(ch + 1);  // in flight under this chunk's MFMAs
        const av_t *wp = reinterpret_cast<const av_t *>(a.itable) + ((int64_t)(ch * G::NW + vw) * G::IK) * 64 + lane;
        // group g of 8 k-steps: k-step kk = 8 g .. 8 g + 7, q = kk >> 5, part = (kk >> 4) & 1, bin pair s = kk & 15
        auto slab = [&](int g) { return Gs + (((g >> 1) & 1) * 32 + 16 * (g & 1) + h) * ID_U + j + 32 * cb0 + (G::Q - 1) - (g >> 2); };
        const float *bp = slab(0);
        gemm_groups<RB, NCB, 8>(acc, wp, bp, 2 * ID_U, G::IK / 8, [&](int g) {
            wp += 8 * 64;
            bp = slab(g + 1);
        });
    }
    const int Ut = a.T + G::Q - 1;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int u = u0 + 32 * (cb0 + cb) + j;
        if (u >= Ut) continue;
        float *__restrict__ o = a.g_pad + ((int64_t)b * Ut + u) * G::HOP;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * (rb0 + rb) + 8 * g + 4 * h;  // registers 4 g .. 4 g + 3 of a lane are four consecutive samples of its hop
                if constexpr (G::HOP % 4 == 0) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[rb][cb][4 * g + e];
                    if (c0 < G::HOP) *reinterpret_cast<f32x4 *>(o + c0) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c0 + e < G::HOP) o[c0 + e] = acc[rb][cb][4 * g + e];
                }
            }
    }
}

// g[j] = (g_p[j + P] + g_p[P - j] for 1 <= j <= P) + g_p[P + 2 (N - 1) - j] for N - 1 - P <= j <= N - 2, P = NFFT / 2; padded sample i is
// g_pad[i - LEFT], 0 outside its (T + Q - 1) HOP samples (no window sample covers those).  g_wav = g, or g_wav + g when a.accumulate.
template <class G>
__global__ void __launch_bounds__(256) stft_fold_kernel(SetStftLossArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= a.N) return;
    const int64_t Lp = (int64_t)(a.T + G::Q - 1) * G::HOP;
    const float *__restrict__ gp = a.g_pad + (int64_t)b * Lp;
    constexpr int P = G::PAD;
    auto at = [&](int64_t i) {
        i -= G::LEFT;
        return i >= 0 && i < Lp ? gp[i] : 0.0f;
    };
    float v = at((int64_t)j + P);
    if (j >= 1 && j <= P) v += at(P - j);
    if (j >= a.N - 1 - P && j <= a.N - 2) v += at((int64_t)P + 2 * ((int64_t)a.N - 1) - j);
    float *__restrict__ o = a.g_wav + (int64_t)b * a.N + j;
    *o = a.accumulate ? *o + v : v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
template <class G>
int stft_sizes(int64_t B, int64_t N, int64_t *out) {
    const int64_t T = 1 + N / G::HOP, tiles = (T + G::TT - 1) / G::TT, Ts = tiles * G::TT, Z = (G::NCH + 3) / 4;
    out[0] = T;
    out[1] = (int64_t)G::NCH * (G::WIN / 2) * 64 * 2;      // table image floats
    out[2] = (int64_t)G::NCH * G::NW * G::IK * 64;         // inverse table image floats
    out[3] = tiles * B * Z * 3;                            // part doubles
    out[4] = B * G::NCH * 32 * Ts;                         // kept magnitudes, floats
    out[5] = 2 * out[4];                                   // spec floats
    out[6] = B * (T + G::Q - 1) * G::HOP;                  // g_pad floats
    out[7] = Ts;
    return SET_OK;
}

template <class G>
int stft_common(const SetStftLossArgs &a, const char *what) {
    SET_REQUIRE(a.B > 0 && a.B <= 65535 && a.N > G::PAD && (int64_t)a.N + G::NFFT < (int64_t)1 << 30, what);
    SET_REQUIRE(a.T == 1 + a.N / G::HOP && a.x_bs >= a.N, what);
    SET_REQUIRE(a.x && a.table && set_aligned16(a.table, nullptr, nullptr), what);
    return SET_OK;
}

template <class G>
int stft_magnitude_launch(const SetStftLossArgs &a, hipStream_t s) {
    if (int rc = stft_common<G>(a, "set_stft_magnitude")) return rc;
    SET_REQUIRE(a.mag != nullptr, "set_stft_magnitude");
    static SetDeviceOnce once;
    if (int rc = set_lds_optin(once, G::LDS, "set_stft_magnitude attr", stft_fwd_kernel<G, 1>)) return rc;
    const int tiles = (a.T + G::TT - 1) / G::TT;
    hipLaunchKernelGGL((stft_fwd_kernel<G, 1>), dim3(tiles, a.B, (G::NCH + 3) / 4), dim3(256), G::LDS, s, a, tiles * G::TT);
    return set_check_launch("set_stft_magnitude");
}

template <class G>
int stft_fwd_launch(const SetStftLossArgs &a, hipStream_t s) {
    if (int rc = stft_common<G>(a, "set_stft_loss_fwd")) return rc;
    SET_REQUIRE(a.y && a.y_bs >= a.N && a.part && a.stats && a.loss && (a.which == 0 || a.which == 1), "set_stft_loss_fwd");
    static SetDeviceOnce once;
    if (int rc = set_lds_optin(once, G::LDS, "set_stft_loss_fwd attr", stft_fwd_kernel<G, 0>)) return rc;
    const int tiles = (a.T + G::TT - 1) / G::TT, Z = (G::NCH + 3) / 4;
    hipLaunchKernelGGL((stft_fwd_kernel<G, 0>), dim3(tiles, a.B, Z), dim3(256), G::LDS, s, a, tiles * G::TT);
    if (int rc = set_check_launch("set_stft_loss_fwd")) return rc;
    hipLaunchKernelGGL(stft_finish_kernel, dim3(1), dim3(256), 0, s, a.part, (int64_t)tiles * a.B * Z, (double)a.B * a.T * G::NBIN, a.stats,
                       a.loss);
    return set_check_launch("set_stft_loss_fwd finish");
}

template <class G>
int stft_bwd_launch(const SetStftLossArgs &a, hipStream_t s) {
    if (int rc = stft_common<G>(a, "set_stft_loss_bwd")) return rc;
    SET_REQUIRE(a.y && a.y_bs >= a.N && a.itable && a.spec && a.g_pad && a.g_wav && (a.g_m || (a.stats && a.u_sc && a.u_mag)), "set_stft_loss_bwd");
    SET_REQUIRE((a.which == 0 || a.which == 1) && (a.accumulate == 0 || a.accumulate == 1), "set_stft_loss_bwd");
    SET_REQUIRE(set_aligned16(a.itable, a.g_pad, nullptr), "set_stft_loss_bwd");
    static SetDeviceOnce once;
    if (int rc = set_lds_optin(once, G::LDS, "set_stft_loss_bwd attr", stft_spec_bwd_kernel<G, false>, stft_spec_bwd_kernel<G, true>)) return rc;
    const int tiles = (a.T + G::TT - 1) / G::TT, Ts = tiles * G::TT;
    const dim3 grid(tiles, a.B, (G::NCH + 3) / 4);
    if (a.mag)
        hipLaunchKernelGGL((stft_spec_bwd_kernel<G, true>), grid, dim3(256), G::LDS, s, a, Ts);
    else
        hipLaunchKernelGGL((stft_spec_bwd_kernel<G, false>), grid, dim3(256), G::LDS, s, a, Ts);
    if (int rc = set_check_launch("set_stft_loss_bwd spectrum")) return rc;
    hipLaunchKernelGGL(stft_idft_kernel<G>, dim3((a.T + G::Q - 1 + G::TT - 1) / G::TT, a.B, G::NW / 4), dim3(256), 0, s, a, Ts);
    if (int rc = set_check_launch("set_stft_loss_bwd inverse")) return rc;
    hipLaunchKernelGGL(stft_fold_kernel<G>, dim3((a.N + 255) / 256, a.B), dim3(256), 0, s, a);
    return set_check_launch("set_stft_loss_bwd fold");
}

// SET_E_UNSUPPORTED with the compiled geometries listed from the table
int stft_unsupported(const char *what) {
    char msg[256];
    int at = snprintf(msg, sizeof(msg), "built for (n_fft, hop, win) =");
#define X(n, h, w) \
    if (at < (int)sizeof(msg)) at += snprintf(msg + at, sizeof(msg) - at, " (%d, %d, %d)", n, h, w);
    STFT_GEOMETRIES(X)
#undef X
    return set_fail(SET_E_UNSUPPORTED, what, msg);
}

}  // namespace

#define STFT_DISPATCH(n, h, w, call) \
    if (n_fft == n && hop == h && win == w) return call<StftGeo<n, h, w>>

extern "C" int64_t set_sizeof_stft_loss_args(void) { return (int64_t)sizeof(SetStftLossArgs); }

extern "C" int32_t set_stft_geometries(int32_t *triples, int32_t max_triples) {
    const int32_t all[] = {
#define X(n, h, w) n, h, w,
        STFT_GEOMETRIES(X)
#undef X
    };
    const int32_t count = (int32_t)(sizeof(all) / sizeof(all[0]) / 3);
    for (int32_t i = 0; triples && i < count && i < max_triples; ++i)
        for (int k = 0; k < 3; ++k) triples[3 * i + k] = all[3 * i + k];
    return count;
}

extern "C" int set_stft_sizes(int32_t n_fft, int32_t hop, int32_t win, int64_t B, int64_t N, int64_t *out8) {
    SET_REQUIRE(out8 != nullptr && B > 0 && N > 0, "set_stft_sizes");
#define X(n, h, w) STFT_DISPATCH(n, h, w, stft_sizes)(B, N, out8);
    STFT_GEOMETRIES(X)
#undef X
    return stft_unsupported("set_stft_sizes");
}

extern "C" int set_stft_magnitude(const SetStftLossArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_stft_magnitude");
    const int n_fft = args->n_fft, hop = args->hop, win = args->win;
#define X(n, h, w) STFT_DISPATCH(n, h, w, stft_magnitude_launch)(*args, (hipStream_t)stream);
    STFT_GEOMETRIES(X)
#undef X
    return stft_unsupported("set_stft_magnitude");
}

extern "C" int set_stft_loss_fwd(const SetStftLossArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_stft_loss_fwd");
    const int n_fft = args->n_fft, hop = args->hop, win = args->win;
#define X(n, h, w) STFT_DISPATCH(n, h, w, stft_fwd_launch)(*args, (hipStream_t)stream);
    STFT_GEOMETRIES(X)
#undef X
    return stft_unsupported("set_stft_loss_fwd");
}

extern "C" int set_stft_loss_bwd(const SetStftLossArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_stft_loss_bwd");
    const int n_fft = args->n_fft, hop = args->hop, win = args->win;
#define X(n, h, w) STFT_DISPATCH(n, h, w, stft_bwd_launch)(*args, (hipStream_t)stream);
    STFT_GEOMETRIES(X)
#undef X
    return stft_unsupported("set_stft_loss_bwd");
}
