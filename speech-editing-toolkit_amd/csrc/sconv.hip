// The multi-period discriminator of HiFi-GAN as the generator step uses it (modules/vocoder/hifigan/hifigan.py:154-223, 301-338):
//   sconv1d_fwd_kernel         strided 1-D convolution with bias and leaky ReLU, implicit GEMM on v_mfma_f32_32x32x2_f32
//   sconv1d_dgrad_kernel       its input gradient, every output phase in one launch, with the gate / add epilogue
//   mpd_fold_conv_*_kernel     the first layer (one input channel) read straight from the two waveforms, and its waveform gradient
//   multi_loss_*_kernel        mean |a - b|, mean (1 - a)^2, mean a^2 over a list of strided tensors, forward and backward
// Activations are [R][C][H] with unit frame stride: every (batch, column) pair of the reference's [B, C, H, p] image is a row of its
// own, so the reference's (K, 1) Conv2d is an ordinary 1-D convolution.  The arithmetic of the two GEMM kernels is that of
// conv1d_mfma_kernel: per output element one fp32 fma chain over (16-channel chunk, tap, channel), products unrounded.
// No atomics; every sum has one order.
#include "weight_image.h"

namespace {

struct SconvArgs {
    const float *x, *w, *bias;
    float *out;
    int R, Cin, Cout, H_in, H_out, K, s, pad, act;
    float slope;
};

// ------------------------------------------------------------------------------------------
// forward.  D[co][h] = sum_{tap, ci} A[co][(tap, ci)] * x[ci][s h + tap - pad].  block = 4 waves as WM (rows) x WN (frames); wave
// tile = 32 rows x 32 NCB frames.  A chunk of KC input channels is staged as [KC][s BN + K - 1] frames (coalesced loads on clamped
// addresses, validity select at the LDS write, two buffers, one barrier per chunk: conv1d.hip); lane l of a half reads frame
// s l + tap: ds_read_b32 banks (s l) % 32 -- distinct for s = 1 and 3, 2-way conflicted for s = 2, 4-way for s = 4.
// A fragments come from the packed image of set_pack_conv_weight (indexed by tap: the stride does not enter it).
// ------------------------------------------------------------------------------------------
template <int S, int WM, int WN, int NCB>
__global__ void __launch_bounds__(256) sconv1d_fwd_kernel(SconvArgs a, int CinP, int RBn, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BN = 32 * NCB * WN;
    constexpr int NJP = (S * BN + 6 + 63) / 64;  // 64-frame column blocks of this stride's widest chunk (K = 7): only those are loaded
    const int Wd = S * BN + a.K - 1;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int r = blockIdx.x / tiles;
    const int h0 = (blockIdx.x - r * tiles) * BN;
    const int rb = blockIdx.y * WM + wm;
    const bool rb_valid = rb < RBn;
    const float *xr = a.x + (int64_t)r * a.Cin * a.H_in;
    const int f0 = S * h0 - a.pad;  // input frame of LDS column 0
    const int cp_total = CinP / 2;

    f32x16 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb] = (f32x16){0};

    float pv[4][NJP];
    auto issue = [&](int c0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cc = min(c0 + wave + 4 * k, a.Cin - 1);
#pragma unroll
            for (int u = 0; u < NJP; ++u) {
                const int fi = f0 + u * 64 + lane;
                pv[k][u] = xr[(int64_t)cc * a.H_in + min(max(fi, 0), a.H_in - 1)];
            }
        }
    };
    auto commit = [&](int boff, int c0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = wave + 4 * k;
            const bool cok = c0 + row < a.Cin;
#pragma unroll
            for (int u = 0; u < NJP; ++u) {
                const int j = u * 64 + lane;
                const int fi = f0 + j;
                if (j < Wd) smem[boff + row * Wd + j] = (cok && fi >= 0 && fi < a.H_in) ? pv[k][u] : 0.0f;
            }
        }
    };
    auto mfmas = [&](int boff, int c0) {
        for (int tap = 0; tap < a.K; ++tap) {
            const float *ap = a.w + (((int64_t)rb * a.K + tap) * cp_total + (c0 >> 1)) * 64 + lane;
            const float *bp = smem + boff + half * Wd + S * (wn * 32 * NCB + l31) + tap;
#pragma unroll
            for (int cp = 0; cp < KC / 2; ++cp) {
                const float av = ap[cp * 64];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma32(av, bp[(2 * cp) * Wd + S * 32 * cb], acc[cb]);
            }
        }
    };
    const int bsz = KC * Wd;
    issue(0);
    commit(0, 0);
    if (KC < CinP) issue(KC);
    __syncthreads();
    int cur = 0;
    for (int c0 = 0; c0 < CinP; c0 += KC, cur = bsz - cur) {
        if (rb_valid) mfmas(cur, c0);
        if (c0 + KC < CinP) {
            commit(bsz - cur, c0 + KC);
            if (c0 + 2 * KC < CinP) issue(c0 + 2 * KC);
        }
        __syncthreads();
    }
    if (!rb_valid) return;
    // epilogue: lanes run along h (coalesced); the bias is fetched as one batch on clamped addresses and selected afterwards, a row
    // or frame outside the output is masked by its offset (BUF_OOB: the store is dropped) -- no branch per element (conv1d.hip)
    const rsrc_t d_out = make_rsrc(a.out + (int64_t)r * a.Cout * a.H_out);
    const rsrc_t d_b = make_rsrc(a.bias ? a.bias : a.w);
    const bool has_bias = a.bias != nullptr;
    const int lrow = rb * 32 + 4 * half;
    const float sl = a.act ? a.slope : 1.0f;
    float bi[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const float bv = buf_load(d_b, (unsigned)min(lrow + urow16(q), a.Cout - 1) * 4u, 0u);
        bi[q] = has_bias ? bv : 0.0f;
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int h = h0 + (wn * NCB + cb) * 32 + l31;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = lrow + urow16(q);
            float v = acc[cb][q] + bi[q];
            v = v > 0.0f ? v : v * sl;
            buf_store(v, d_out, (co < a.Cout && h < a.H_out) ? (unsigned)(co * a.H_out + h) * 4u : BUF_OOB, 0u);
        }
    }
}

// ------------------------------------------------------------------------------------------
// input gradient.  dz_in[ci][j] = gate(f_in[ci][j]) (add[ci][j] + sum_{co, k} W[co][ci][k] dz_out[co][(j + pad - k) / s]) over the
// taps with (j + pad - k) % s == 0.  Rows of the GEMM are the input channels ci (the image is that of the transposed weight), the
// reduction runs over (co, k).  A tile is S QB consecutive frames j = S (q0 + q) + phi, held PHASE-MAJOR: the 32 columns of one MFMA
// share phi, so they share their taps k = k0 + S m (k0 = (phi + pad) % S) and read dz_out frame q0 + q + e - m (e = (phi + pad) / S):
// a stride-1 read of the staged [KC][QB + MH + EH] frames.  Every tap belongs to one phase: an A fragment is loaded once per chunk.
// Epilogue: the accumulators go through LDS eight rows per wave at a time, written at column S q + phi and read back along j, so
// f_in, add and dz_in are accessed in whole rows (no stride-S scatter).
// ------------------------------------------------------------------------------------------
struct SdgradArgs {
    const float *dz_out, *w, *f_in, *add;
    float *dz_in;
    int R, Cin, Cout, H_in, H_out, K, pad;
    float slope;
};

template <int S, int NQ>
__global__ void __launch_bounds__(256) sconv1d_dgrad_kernel(SdgradArgs a, int CoP, int RBn, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QB = 32 * NQ, JW = S * QB;
    const int MH = (a.K - 1) / S, EH = (S - 1 + a.pad) / S;
    const int Wd = QB + MH + EH;  // <= 44 (NQ = 1) / 76 (NQ = 2): NQ column blocks of 64
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int r = blockIdx.x / tiles;
    const int q0 = (blockIdx.x - r * tiles) * QB;
    const int rb = blockIdx.y * 4 + wave;
    const bool rb_valid = rb < RBn;
    const float *gr = a.dz_out + (int64_t)r * a.Cout * a.H_out;
    const int t0 = q0 - MH;  // dz_out frame of LDS column 0
    const int cp_total = CoP / 2;

    f32x16 acc[S * NQ];
#pragma unroll
    for (int i = 0; i < S * NQ; ++i) acc[i] = (f32x16){0};

    float pv[4][NQ];
    auto issue = [&](int c0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cc = min(c0 + wave + 4 * k, a.Cout - 1);
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const int t = t0 + u * 64 + lane;
                pv[k][u] = gr[(int64_t)cc * a.H_out + min(max(t, 0), a.H_out - 1)];
            }
        }
    };
    auto commit = [&](int boff, int c0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = wave + 4 * k;
            const bool cok = c0 + row < a.Cout;
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const int j = u * 64 + lane;
                const int t = t0 + j;
                if (j < Wd) smem[boff + row * Wd + j] = (cok && t >= 0 && t < a.H_out) ? pv[k][u] : 0.0f;
            }
        }
    };
    auto mfmas = [&](int boff, int c0) {
        auto phase = [&](auto PHI) __attribute__((always_inline)) {
            constexpr int phi = decltype(PHI)::value;
            const int k0 = (phi + a.pad) % S, e = (phi + a.pad) / S;
            for (int k = k0, m = 0; k < a.K; k += S, ++m) {
                const float *ap = a.w + (((int64_t)rb * a.K + k) * cp_total + (c0 >> 1)) * 64 + lane;
                const float *bp = smem + boff + half * Wd + l31 + e - m + MH;
#pragma unroll
                for (int cp = 0; cp < KC / 2; ++cp) {
                    const float av = ap[cp * 64];
#pragma unroll
                    for (int nq = 0; nq < NQ; ++nq) acc[phi * NQ + nq] = mfma32(av, bp[(2 * cp) * Wd + 32 * nq], acc[phi * NQ + nq]);
                }
            }
        };
        phase(ic<0>{});
        if constexpr (S > 1) phase(ic<1>{});
        if constexpr (S > 2) phase(ic<2>{});
        if constexpr (S > 3) phase(ic<3>{});
    };
    const int bsz = KC * Wd;
    issue(0);
    commit(0, 0);
    if (KC < CoP) issue(KC);
    __syncthreads();
    int cur = 0;
    for (int c0 = 0; c0 < CoP; c0 += KC, cur = bsz - cur) {
        if (rb_valid) mfmas(cur, c0);
        if (c0 + KC < CoP) {
            commit(bsz - cur, c0 + KC);
            if (c0 + 2 * KC < CoP) issue(c0 + 2 * KC);
        }
        __syncthreads();
    }
    // epilogue (every wave: the barriers are the block's).  Optional operands are loaded from a valid dummy address and selected.
    const bool has_gate = a.f_in != nullptr, has_add = a.add != nullptr;
    const int64_t rbase = (int64_t)r * a.Cin * a.H_in;
    const float *fp = has_gate ? a.f_in + rbase : gr;
    const float *dp = has_add ? a.add + rbase : gr;
    const rsrc_t d_in = make_rsrc(a.dz_in + rbase);
    const int j0 = S * q0;
    float *mine = smem + wave * 8 * JW;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        __syncthreads();  // the staged chunk / the previous group's rows are consumed
#pragma unroll
        for (int i = 0; i < S * NQ; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) mine[(4 * half + q) * JW + S * (l31 + 32 * (i % NQ)) + i / NQ] = acc[i][4 * g + q];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < (JW + 63) / 64; ++u) {
            const int jj = u * 64 + lane;
            const int j = j0 + jj;
            const bool jv = jj < JW && j < a.H_in;
            const int jl = jv ? jj : 0;
            float fv[8], av[8];
            int idx[8];
#pragma unroll
            for (int row = 0; row < 8; ++row) {
                const int ci = rb * 32 + 8 * g + row;
                const bool v = rb_valid && ci < a.Cin && jv;
                idx[row] = v ? ci * a.H_in + j : -1;
                fv[row] = fp[has_gate && v ? idx[row] : 0];
                av[row] = dp[has_add && v ? idx[row] : 0];
            }
#pragma unroll
            for (int row = 0; row < 8; ++row) {
                const float gate = has_gate ? (fv[row] > 0.0f ? 1.0f : a.slope) : 1.0f;
                const float v = (mine[row * JW + jl] + (has_add ? av[row] : 0.0f)) * gate;
                buf_store(v, d_in, idx[row] >= 0 ? (unsigned)idx[row] * 4u : BUF_OOB, 0u);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// first layer, forward: one wave = 64 frames h of one row (signal, b, w); the K input samples are read once (through the right
// reflect pad: position n >= T reads 2 (T - 1) - n), then every output channel is one fma chain over k ascending from 0, + bias.
// Memory-bound on the [R][C][H_out] store (coalesced along h).
// ------------------------------------------------------------------------------------------
constexpr int FOLD_KMAX = 7;

__global__ void __launch_bounds__(256) mpd_fold_conv_fwd_kernel(const float *y, const float *y_hat, const float *w, const float *bias, float *out,
                                                                int B, int T, int p, int C, int K, int s, int pad, int H_in, int H_out,
                                                                int tiles, int act, float slope, int64_t units) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= units) return;
    const int row = (int)(unit / tiles);
    const int h = (int)(unit - (int64_t)row * tiles) * 64 + lane;
    const int sig = row / (B * p), bw = row - sig * B * p;
    const int b = bw / p, wc = bw - b * p;
    const float *src = (sig ? y_hat : y) + (int64_t)b * T;
    float xv[FOLD_KMAX];
#pragma unroll
    for (int k = 0; k < FOLD_KMAX; ++k) {
        const int i = s * h + k - pad;
        const bool ok = k < K && h < H_out && i >= 0 && i < H_in;
        const int n = ok ? i * p + wc : 0;
        const float v = src[n < T ? n : 2 * (T - 1) - n];
        xv[k] = ok ? v : 0.0f;
    }
    const float sl = act ? slope : 1.0f;
    float *o = out + (int64_t)row * C * H_out + h;
    for (int c = 0; c < C; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < FOLD_KMAX; ++k)
            if (k < K) acc = fmaf(w[c * K + k], xv[k], acc);
        float v = acc + (bias ? bias[c] : 0.0f);
        v = v > 0.0f ? v : v * sl;
        if (h < H_out) o[(int64_t)c * H_out] = v;
    }
}

// first layer, backward: the gradient at padded position (row i, column w) of batch b's generated signal,
//   G(i, w) = fma chain over c ascending, inside it k ascending, of W[c][k] dz[(b p + w)][c][(i + pad - k) / s]
// (taps that are not a multiple of s away from an output frame, or whose frame is outside [0, H_out), add an exact 0), and
//   g_wav[b][n] = G(n / p, n % p) + G(m / p, m % p)  with the second term only when the mirror m = 2 (T - 1) - n is in [T, Tp).
// One wave = 64 rows i of one (b, w): dz is read along h.
__device__ __forceinline__ float mpd_fold_g(const float *dzr, const float *w, int i, int C, int K, int s, int pad, int H_out) {
    int hh[FOLD_KMAX];
    bool ok[FOLD_KMAX];
#pragma unroll
    for (int k = 0; k < FOLD_KMAX; ++k) {
        const int num = i + pad - k;
        const int q = num / s;
        ok[k] = k < K && num >= 0 && q * s == num && q < H_out;
        hh[k] = ok[k] ? q : 0;
    }
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float *dc = dzr + (int64_t)c * H_out;
#pragma unroll
        for (int k = 0; k < FOLD_KMAX; ++k) {
            if (k < K) {  // uniform
                const float v = dc[hh[k]];
                acc = fmaf(w[c * K + k], ok[k] ? v : 0.0f, acc);
            }
        }
    }
    return acc;
}

__global__ void __launch_bounds__(256) mpd_fold_conv_bwd_kernel(const float *dz, const float *w, float *g_wav, int B, int T, int p, int C, int K,
                                                                int s, int pad, int H_in, int H_out, int tiles, int64_t units) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= units) return;
    const int bw = (int)(unit / tiles);
    const int i = (int)(unit - (int64_t)bw * tiles) * 64 + lane;
    const int b = bw / p, wc = bw - b * p;
    const int n = i * p + wc;
    if (i >= H_in || n >= T) return;
    const int64_t rs = (int64_t)C * H_out;
    float g = mpd_fold_g(dz + (int64_t)bw * rs, w, i, C, K, s, pad, H_out);
    const int m = 2 * (T - 1) - n;
    if (m >= T && m < H_in * p) {  // at most p - 1 samples per signal
        const int im = m / p, wm = m - im * p;
        g += mpd_fold_g(dz + ((int64_t)b * p + wm) * rs, w, im, C, K, s, pad, H_out);
    }
    g_wav[(int64_t)b * T + n] = g;
}

// ------------------------------------------------------------------------------------------
// the three loss forms over a list of items.  An item is SET_MULTI_LOSS_WORDS 64-bit words (include/set_amd.h).  Element li of an
// item is the row-major index over its four extents; a chunk is SET_MULTI_LOSS_CHUNK consecutive elements.
//   block partial: thread t adds the terms of elements chunk + t + 256 u, u = 0 .. 7 ascending, in double, then the 256 thread
//   sums are halved pairwise (red[t] += red[t + st], st = 128 .. 1);
//   item sum: thread t of the one finishing block adds the item's partials t, t + 256, .. ascending, then the same halving;
//   result: thread 0 adds sum / numel of the items of a slot in list order, multiplies by scale and rounds once to fp32.
// ------------------------------------------------------------------------------------------
constexpr int ML_W = SET_MULTI_LOSS_WORDS, ML_CHUNK = SET_MULTI_LOSS_CHUNK, ML_SLOTS = 4;
static_assert(ML_CHUNK == 256 * 8, "a chunk is eight elements per thread");

struct MlItem {
    const float *a, *b;
    float *g;
    int mode, slot;
    int64_t e[4], sa[4], sb[4], chunk0, numel;
};
__device__ __forceinline__ MlItem ml_item(const int64_t *items, int i) {
    const int64_t *w = items + (int64_t)i * ML_W;
    MlItem it;
    it.a = reinterpret_cast<const float *>(w[0]);
    it.b = reinterpret_cast<const float *>(w[1]);
    it.g = reinterpret_cast<float *>(w[2]);
    it.mode = (int)w[3];
#pragma unroll
    for (int d = 0; d < 4; ++d) { it.e[d] = w[4 + d]; it.sa[d] = w[8 + d]; it.sb[d] = w[12 + d]; }
    it.chunk0 = w[16];
    it.slot = (int)w[17];
    it.numel = it.e[0] * it.e[1] * it.e[2] * it.e[3];
    return it;
}
// the item of a chunk: the last one whose first chunk is not behind it (chunk0 ascends with the list)
__device__ __forceinline__ int ml_find(const int64_t *items, int n_items, int64_t chunk) {
    int i = 0;
    while (i + 1 < n_items && items[(int64_t)(i + 1) * ML_W + 16] <= chunk) ++i;
    return i;
}
__device__ __forceinline__ void ml_offsets(const MlItem &it, int64_t li, int64_t &oa, int64_t &ob) {
    const int64_t i3 = li % it.e[3], r2 = li / it.e[3];
    const int64_t i2 = r2 % it.e[2], r1 = r2 / it.e[2];
    const int64_t i1 = r1 % it.e[1], i0 = r1 / it.e[1];
    oa = i0 * it.sa[0] + i1 * it.sa[1] + i2 * it.sa[2] + i3 * it.sa[3];
    ob = i0 * it.sb[0] + i1 * it.sb[1] + i2 * it.sb[2] + i3 * it.sb[3];
}
__device__ __forceinline__ double ml_block_sum(double s, double *red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    const double tot = red[0];
    __syncthreads();
    return tot;
}

__global__ void __launch_bounds__(256) multi_loss_part_kernel(const int64_t *items, int n_items, double *part) {
    __shared__ double red[256];
    const int64_t chunk = blockIdx.x;
    const MlItem it = ml_item(items, ml_find(items, n_items, chunk));
    const int64_t base = (chunk - it.chunk0) * ML_CHUNK + threadIdx.x;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int64_t li = base + 256 * u;
        if (li < it.numel) {
            int64_t oa, ob;
            ml_offsets(it, li, oa, ob);
            const double av = (double)it.a[oa];
            double t;
            if (it.mode == SET_LOSS_L1) t = fabs(av - (double)it.b[ob]);
            else if (it.mode == SET_LOSS_SQ1) t = (1.0 - av) * (1.0 - av);
            else t = av * av;
            s += t;
        }
    }
    const double tot = ml_block_sum(s, red);
    if (threadIdx.x == 0) part[chunk] = tot;
}

__global__ void __launch_bounds__(256) multi_loss_finish_kernel(const int64_t *items, int n_items, int64_t total_chunks, const double *part,
                                                                float scale, int n_slots, float *loss) {
    __shared__ double red[256];
    double tot[ML_SLOTS] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n_items; ++i) {
        const MlItem it = ml_item(items, i);
        const int64_t c1 = i + 1 < n_items ? items[(int64_t)(i + 1) * ML_W + 16] : total_chunks;
        double s = 0.0;
        for (int64_t c = it.chunk0 + threadIdx.x; c < c1; c += 256) s += part[c];
        const double sum = ml_block_sum(s, red);
#pragma unroll
        for (int k = 0; k < ML_SLOTS; ++k)
            if (k == it.slot) tot[k] += sum / (double)it.numel;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < ML_SLOTS; ++k)
            if (k < n_slots) loss[k] = (float)(tot[k] * (double)scale);
    }
}

// grad_a = coef * {sign(a - b), 2 (a - 1), 2 a},  coef = fp32(u[slot] * scale / numel) (the product and quotient in double)
__global__ void __launch_bounds__(256) multi_loss_bwd_kernel(const int64_t *items, int n_items, const float *u, float scale) {
    const int64_t chunk = blockIdx.x;
    const MlItem it = ml_item(items, ml_find(items, n_items, chunk));
    if (it.g == nullptr) return;
    const float coef = (float)((double)u[it.slot] * (double)scale / (double)it.numel);
    const int64_t base = (chunk - it.chunk0) * ML_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t li = base + 256 * k;
        if (li < it.numel) {
            int64_t oa, ob;
            ml_offsets(it, li, oa, ob);
            const float av = it.a[oa];
            float d;
            if (it.mode == SET_LOSS_L1) {
                const float df = av - it.b[ob];
                d = df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : 0.0f);
            } else if (it.mode == SET_LOSS_SQ1) {
                d = 2.0f * (av - 1.0f);
            } else {
                d = 2.0f * av;
            }
            it.g[oa] = coef * d;
        }
    }
}

bool sconv_shape_ok(int R, int Cin, int Cout, int H_in, int K, int s, int pad) {
    return R > 0 && Cin > 0 && Cout > 0 && H_in > 0 && K >= 1 && K <= 7 && s >= 1 && s <= 4 && pad >= 0 && pad < K;
}
inline int sconv_out_len(int H_in, int K, int s, int pad) { return H_in + 2 * pad >= K ? (H_in + 2 * pad - K) / s + 1 : 0; }
constexpr int64_t SLICE_LIMIT = (int64_t)1 << 29;  // floats: one row's [C][H] slice is addressed with 32-bit byte offsets

}  // namespace

extern "C" int32_t set_sconv1d_out_len(int32_t H_in, int32_t K, int32_t s, int32_t pad) {
    if (!sconv_shape_ok(1, 1, 1, H_in, K, s, pad)) return set_fail(SET_E_INVALID, "set_sconv1d_out_len", "needs H_in > 0, 1 <= K <= 7, 1 <= s <= 4, 0 <= pad < K");
    return sconv_out_len(H_in, K, s, pad);
}

extern "C" int set_sconv1d_fwd(const float *x, const float *wp, const float *bias, float *out, int32_t R, int32_t Cin, int32_t Cout, int32_t H_in,
                               int32_t K, int32_t s, int32_t pad, int32_t act, float slope, void *stream) {
    SET_REQUIRE(x && wp && out, "set_sconv1d_fwd");
    SET_REQUIRE(sconv_shape_ok(R, Cin, Cout, H_in, K, s, pad), "set_sconv1d_fwd");
    SET_REQUIRE(act == 0 || act == 1, "set_sconv1d_fwd");
    const int H_out = sconv_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, "set_sconv1d_fwd");
    if ((int64_t)Cin * H_in >= SLICE_LIMIT || (int64_t)Cout * H_out >= SLICE_LIMIT)
        return set_fail(SET_E_UNSUPPORTED, "set_sconv1d_fwd", "one row's [C][H] slice exceeds 2 GiB");
    const int CinP = set_round_up(Cin, KC), RBn = (Cout + 31) / 32;
    SconvArgs a{x, wp, bias, out, R, Cin, Cout, H_in, H_out, K, s, pad, act, slope};
    auto launch = [&](auto S_, auto WM_, auto WN_, auto NCB_) {
        constexpr int S = decltype(S_)::value, WM = decltype(WM_)::value, WN = decltype(WN_)::value, NCB = decltype(NCB_)::value, BN = 32 * NCB * WN;
        const int tiles = (H_out + BN - 1) / BN;
        if ((int64_t)R * tiles > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_sconv1d_fwd", "more than 2^31 - 1 tiles");
        const size_t lds = (size_t)2 * KC * (s * BN + K - 1) * sizeof(float);
        hipLaunchKernelGGL((sconv1d_fwd_kernel<S, WM, WN, NCB>), dim3((unsigned)(R * tiles), (RBn + WM - 1) / WM), dim3(256), lds, (hipStream_t)stream, a,
                           CinP, RBn, tiles);
        return set_check_launch("set_sconv1d_fwd");
    };
    // 32-frame tiles for short rows (the last layers of the long periods have 10 - 30 frames), else 64; flat layers put two waves
    // along the frames
    auto shape = [&](auto S_) {
        if (H_out <= 32) return launch(S_, ic<4>{}, ic<1>{}, ic<1>{});
        if (RBn >= 3) return launch(S_, ic<4>{}, ic<1>{}, ic<2>{});
        return launch(S_, ic<2>{}, ic<2>{}, ic<1>{});
    };
    // the stride is a template parameter: the staging loads and their registers are sized for it, not for s = 4
    if (s == 1) return shape(ic<1>{});
    if (s == 2) return shape(ic<2>{});
    if (s == 3) return shape(ic<3>{});
    return shape(ic<4>{});
}

extern "C" int set_sconv1d_dgrad(const float *dz_out, const float *wtp, const float *f_in, const float *add, float *dz_in, int32_t R, int32_t Cin,
                                 int32_t Cout, int32_t H_in, int32_t K, int32_t s, int32_t pad, float slope, void *stream) {
    SET_REQUIRE(dz_out && wtp && dz_in, "set_sconv1d_dgrad");
    SET_REQUIRE(sconv_shape_ok(R, Cin, Cout, H_in, K, s, pad), "set_sconv1d_dgrad");
    const int H_out = sconv_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, "set_sconv1d_dgrad");
    if ((int64_t)Cin * H_in >= SLICE_LIMIT || (int64_t)Cout * H_out >= SLICE_LIMIT)
        return set_fail(SET_E_UNSUPPORTED, "set_sconv1d_dgrad", "one row's [C][H] slice exceeds 2 GiB");
    const int CoP = set_round_up(Cout, KC), RBn = (Cin + 31) / 32;
    SdgradArgs a{dz_out, wtp, f_in, add, dz_in, R, Cin, Cout, H_in, H_out, K, pad, slope};
    auto launch = [&](auto S_, auto NQ_) {
        constexpr int S = decltype(S_)::value, NQ = decltype(NQ_)::value, JW = S * 32 * NQ;
        const int tiles = (H_in + JW - 1) / JW;
        if ((int64_t)R * tiles > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_sconv1d_dgrad", "more than 2^31 - 1 tiles");
        const size_t stage = (size_t)2 * KC * (32 * NQ + (K - 1) / S + (S - 1 + pad) / S) * sizeof(float), epi = (size_t)4 * 8 * JW * sizeof(float);
        hipLaunchKernelGGL((sconv1d_dgrad_kernel<S, NQ>), dim3((unsigned)(R * tiles), (RBn + 3) / 4), dim3(256), stage > epi ? stage : epi,
                           (hipStream_t)stream, a, CoP, RBn, tiles);
        return set_check_launch("set_sconv1d_dgrad");
    };
    if (s == 1) return H_in <= 32 ? launch(ic<1>{}, ic<1>{}) : launch(ic<1>{}, ic<2>{});
    if (s == 2) return launch(ic<2>{}, ic<1>{});
    if (s == 3) return launch(ic<3>{}, ic<1>{});
    return launch(ic<4>{}, ic<1>{});
}

static bool fold_shape_ok(int B, int T, int p, int C, int K, int s, int pad) {
    return B > 0 && p >= 1 && T > p && T <= (1 << 30) && C > 0 && K >= 1 && K <= FOLD_KMAX && s >= 1 && s <= 4 && pad >= 0 && pad < K &&
           (int64_t)B * p <= (1 << 30);
}

extern "C" int set_mpd_fold_conv_fwd(const float *y, const float *y_hat, const float *w, const float *bias, float *out, int32_t B, int32_t T, int32_t p,
                                     int32_t C, int32_t K, int32_t s, int32_t pad, int32_t act, float slope, void *stream) {
    SET_REQUIRE(y && y_hat && w && out, "set_mpd_fold_conv_fwd");
    SET_REQUIRE(fold_shape_ok(B, T, p, C, K, s, pad), "set_mpd_fold_conv_fwd");
    SET_REQUIRE(act == 0 || act == 1, "set_mpd_fold_conv_fwd");
    const int H_in = (T + p - 1) / p, H_out = sconv_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, "set_mpd_fold_conv_fwd");
    const int tiles = (H_out + 63) / 64;
    const int64_t units = (int64_t)2 * B * p * tiles;
    if ((units + 3) / 4 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_mpd_fold_conv_fwd", "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(mpd_fold_conv_fwd_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, y_hat, w, bias, out, B, T, p, C, K,
                       s, pad, H_in, H_out, tiles, act, slope, units);
    return set_check_launch("set_mpd_fold_conv_fwd");
}

extern "C" int set_mpd_fold_conv_bwd(const float *dz, const float *w, float *g_wav, int32_t B, int32_t T, int32_t p, int32_t C, int32_t K, int32_t s,
                                     int32_t pad, void *stream) {
    SET_REQUIRE(dz && w && g_wav, "set_mpd_fold_conv_bwd");
    SET_REQUIRE(fold_shape_ok(B, T, p, C, K, s, pad), "set_mpd_fold_conv_bwd");
    const int H_in = (T + p - 1) / p, H_out = sconv_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, "set_mpd_fold_conv_bwd");
    const int tiles = (H_in + 63) / 64;
    const int64_t units = (int64_t)B * p * tiles;
    if ((units + 3) / 4 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_mpd_fold_conv_bwd", "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(mpd_fold_conv_bwd_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dz, w, g_wav, B, T, p, C, K, s, pad,
                       H_in, H_out, tiles, units);
    return set_check_launch("set_mpd_fold_conv_bwd");
}

extern "C" int set_multi_loss_fwd(const int64_t *items, int32_t n_items, int64_t total_chunks, float scale, int32_t n_slots, double *part, float *loss,
                                  void *stream) {
    SET_REQUIRE(items && part && loss, "set_multi_loss_fwd");
    SET_REQUIRE(n_items > 0 && total_chunks >= n_items && total_chunks <= 0x7fffffff && n_slots >= 1 && n_slots <= ML_SLOTS, "set_multi_loss_fwd");
    hipLaunchKernelGGL(multi_loss_part_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, items, n_items, part);
    hipLaunchKernelGGL(multi_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, items, n_items, total_chunks, part, scale, n_slots, loss);
    return set_check_launch("set_multi_loss_fwd");
}

extern "C" int set_multi_loss_bwd(const int64_t *items, int32_t n_items, int64_t total_chunks, float scale, const float *u, void *stream) {
    SET_REQUIRE(items && u, "set_multi_loss_bwd");
    SET_REQUIRE(n_items > 0 && total_chunks >= n_items && total_chunks <= 0x7fffffff, "set_multi_loss_bwd");
    hipLaunchKernelGGL(multi_loss_bwd_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, items, n_items, u, scale);
    return set_check_launch("set_multi_loss_bwd");
}
