// The multi-scale discriminator of HiFi-GAN as the generator step uses it (modules/vocoder/hifigan/hifigan.py:226-298):
//   gconv1d_fwd_kernel      grouped strided 1-D convolution (K <= 41) with bias and leaky ReLU, implicit GEMM on v_mfma_f32_32x32x2_f32
//   gconv1d_dgrad_kernel    its input gradient, every output phase in one launch, with the gate / add epilogue
//   wave_conv_*_kernel      the first layer (one input channel, stride 1) straight from the two waveforms, and its waveform gradient
//   avgpool4s2_*_kernel     AvgPool1d(4, 2, padding = 1) on [B][T] and its transpose with an add operand
// Activations are [R][C][H] rows as in sconv.hip.  A block works on ONE group: its x window is staged in LDS per 16-channel chunk and
// serves every output channel of the group and every tap, so a layer reads x once (Cout / g <= 64; beyond that once per 64 rows).
// The packed weight is `groups` images of set_pack_conv_weight, one [Cout / g][Cin / g][K] dense weight each, back to back.
// Arithmetic: per output element one fp32 fma chain over (16-channel chunk, tap, channel), products unrounded.  No atomics.
#include "weight_image.h"

namespace {

constexpr int GCONV_KMAX = SET_GCONV_KMAX;

struct GconvArgs {
    const float *x, *w, *bias;
    float *out;
    int R, Cin_g, Cout_g, groups, H_in, H_out, K, pad, act;
    float slope;
};

// ------------------------------------------------------------------------------------------
// forward.  block = 4 waves as WM (32-row blocks of the group) x WN (32-frame column blocks): BN = 32 WN output frames of one row r and
// one group.  The window of a chunk is the S BN + K - 1 input frames from f0 = S h0 - pad, staged DE-INTERLEAVED BY PHASE: frame
// f0 + j sits at column (j % S) PW + j / S of its channel's line, PW = BN + (K - 1) / S.  The B operand of (frame h0 + n, tap) is frame
// j = S n + tap = column (tap % S) PW + tap / S + n: the 32 lanes of a ds_read_b32 group read 32 consecutive dwords whatever S is.
// Global reads run along j (coalesced); the LDS writes are S-way strided (ds_write_b32: 2-way is free, S = 4 costs 2 x on 1 / K-th of
// the traffic).  Columns past the window and channels past Cin / g are written as zeros: every staged dword is defined.
// ------------------------------------------------------------------------------------------
template <int S, int WM, int WN>
__global__ void __launch_bounds__(256) gconv1d_fwd_kernel(GconvArgs a, int CinP, int RBn, int RBY, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BN = 32 * WN;
    const int PW = BN + (a.K - 1) / S;
    const int Wd = S * PW;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int r = blockIdx.x / tiles;
    const int h0 = (blockIdx.x - r * tiles) * BN;
    const int g = blockIdx.y / RBY;
    const int rb = (blockIdx.y - g * RBY) * WM + wm;  // 32-row block inside the group
    const bool rb_valid = rb < RBn;
    const float *xg = a.x + ((int64_t)r * a.groups + g) * a.Cin_g * a.H_in;
    const float *wg = a.w + (int64_t)g * RBn * 32 * a.K * CinP;
    const int f0 = S * h0 - a.pad;
    const int cp_total = CinP / 2;
    const int Wj = S * BN + a.K - 1;  // frames of the window

    f32x16 acc = (f32x16){0};
    for (int c0 = 0; c0 < CinP; c0 += KC) {
        __syncthreads();  // the previous chunk is consumed
        for (int row = wave; row < KC; row += 4) {
            const bool cok = c0 + row < a.Cin_g;
            const float *xc = xg + (int64_t)min(c0 + row, a.Cin_g - 1) * a.H_in;
            for (int j = lane; j < Wd; j += 64) {
                const int fi = f0 + j;
                const float v = xc[min(max(fi, 0), a.H_in - 1)];
                smem[row * Wd + (j % S) * PW + j / S] = (cok && j < Wj && fi >= 0 && fi < a.H_in) ? v : 0.0f;
            }
        }
        __syncthreads();
        if (rb_valid) {
            for (int tap = 0; tap < a.K; ++tap) {
                const float *ap = wg + (((int64_t)rb * a.K + tap) * cp_total + (c0 >> 1)) * 64 + lane;
                const float *bp = smem + half * Wd + (tap % S) * PW + tap / S + wn * 32 + l31;
#pragma unroll
                for (int cp = 0; cp < KC / 2; ++cp) acc = mfma32(ap[cp * 64], bp[(2 * cp) * Wd], acc);
            }
        }
    }
    if (!rb_valid) return;
    const int64_t obase = ((int64_t)r * a.groups + g) * a.Cout_g * a.H_out;
    const rsrc_t d_out = make_rsrc(a.out + obase);
    const bool has_bias = a.bias != nullptr;
    const float *bg = has_bias ? a.bias + g * a.Cout_g : a.w;
    const int lrow = rb * 32 + 4 * half;
    const float sl = a.act ? a.slope : 1.0f;
    const int h = h0 + wn * 32 + l31;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int co = lrow + urow16(q);
        const float bv = bg[has_bias ? min(co, a.Cout_g - 1) : 0];
        float v = acc[q] + (has_bias ? bv : 0.0f);
        v = v > 0.0f ? v : v * sl;
        buf_store(v, d_out, (co < a.Cout_g && h < a.H_out) ? (unsigned)(co * a.H_out + h) * 4u : BUF_OOB, 0u);
    }
}

// ------------------------------------------------------------------------------------------
// input gradient, as sconv1d_dgrad_kernel: rows are the group's input channels (the images are those of the group's transposed
// weights), the reduction runs over (co of the group, k).  A block owns S QB consecutive frames j = S (q0 + q) + phi of one row and one
// group, QB = 32 WN; wave (wm, wn) holds the S phases of the 32 columns q = 32 wn + l.  Columns of one MFMA share phi, hence their taps
// k = k0 + S m and the dz_out frame q0 + q + e - m: stride-1 reads of the staged [KC][QB + MH + EH] frames, conflict-free at every S.
// Epilogue through LDS (eight rows per wave at a time, written at column S l + phi, read back along j): f_in, add and dz_in are
// accessed in whole rows.
// ------------------------------------------------------------------------------------------
struct GdgradArgs {
    const float *dz_out, *w, *f_in, *add;
    float *dz_in;
    int R, Cin_g, Cout_g, groups, H_in, H_out, K, pad;
    float slope;
};

template <int S, int WM, int WN>
__global__ void __launch_bounds__(256) gconv1d_dgrad_kernel(GdgradArgs a, int CoP, int RBn, int RBY, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QB = 32 * WN, JWW = S * 32;  // JWW: the frames of one wave's columns
    const int MH = (a.K - 1) / S, EH = (S - 1 + a.pad) / S;
    const int Wd = QB + MH + EH;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int r = blockIdx.x / tiles;
    const int q0 = (blockIdx.x - r * tiles) * QB;
    const int g = blockIdx.y / RBY;
    const int rb = (blockIdx.y - g * RBY) * WM + wm;
    const bool rb_valid = rb < RBn;
    const float *gr = a.dz_out + ((int64_t)r * a.groups + g) * a.Cout_g * a.H_out;
    const float *wg = a.w + (int64_t)g * RBn * 32 * a.K * CoP;
    const int t0 = q0 - MH;  // dz_out frame of LDS column 0
    const int cp_total = CoP / 2;

    f32x16 acc[S];
#pragma unroll
    for (int i = 0; i < S; ++i) acc[i] = (f32x16){0};

    for (int c0 = 0; c0 < CoP; c0 += KC) {
        __syncthreads();
        for (int row = wave; row < KC; row += 4) {
            const bool cok = c0 + row < a.Cout_g;
            const float *gc = gr + (int64_t)min(c0 + row, a.Cout_g - 1) * a.H_out;
            for (int j = lane; j < Wd; j += 64) {
                const int t = t0 + j;
                const float v = gc[min(max(t, 0), a.H_out - 1)];
                smem[row * Wd + j] = (cok && t >= 0 && t < a.H_out) ? v : 0.0f;
            }
        }
        __syncthreads();
        if (rb_valid) {
            auto phase = [&](auto PHI) __attribute__((always_inline)) {
                constexpr int phi = decltype(PHI)::value;
                const int k0 = (phi + a.pad) % S, e = (phi + a.pad) / S;
                for (int k = k0, m = 0; k < a.K; k += S, ++m) {
                    const float *ap = wg + (((int64_t)rb * a.K + k) * cp_total + (c0 >> 1)) * 64 + lane;
                    const float *bp = smem + half * Wd + wn * 32 + l31 + e - m + MH;
#pragma unroll
                    for (int cp = 0; cp < KC / 2; ++cp) acc[phi] = mfma32(ap[cp * 64], bp[(2 * cp) * Wd], acc[phi]);
                }
            };
            phase(ic<0>{});
            if constexpr (S > 1) phase(ic<1>{});
            if constexpr (S > 2) phase(ic<2>{});
            if constexpr (S > 3) phase(ic<3>{});
        }
    }
    // epilogue (every wave: the barriers are the block's).  Optional operands are loaded from a valid dummy address and selected.
    const bool has_gate = a.f_in != nullptr, has_add = a.add != nullptr;
    const int64_t rbase = ((int64_t)r * a.groups + g) * a.Cin_g * a.H_in;
    const float *fp = has_gate ? a.f_in + rbase : gr;
    const float *dp = has_add ? a.add + rbase : gr;
    const rsrc_t d_in = make_rsrc(a.dz_in + rbase);
    const int j0 = S * (q0 + wn * 32);
    float *mine = smem + wave * 8 * JWW;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        __syncthreads();  // the staged chunk / the previous group's rows are consumed
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) mine[(4 * half + q) * JWW + S * l31 + i] = acc[i][4 * gq + q];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < (JWW + 63) / 64; ++u) {
            const int jj = u * 64 + lane;
            const int j = j0 + jj;
            const bool jv = jj < JWW && j < a.H_in;
            const int jl = jv ? jj : 0;
            float fv[8], av[8];
            int idx[8];
#pragma unroll
            for (int row = 0; row < 8; ++row) {
                const int ci = rb * 32 + 8 * gq + row;
                const bool v = rb_valid && ci < a.Cin_g && jv;
                idx[row] = v ? ci * a.H_in + j : -1;
                fv[row] = fp[has_gate && v ? idx[row] : 0];
                av[row] = dp[has_add && v ? idx[row] : 0];
            }
#pragma unroll
            for (int row = 0; row < 8; ++row) {
                const float gate = has_gate ? (fv[row] > 0.0f ? 1.0f : a.slope) : 1.0f;
                const float v = (mine[row * JWW + jl] + (has_add ? av[row] : 0.0f)) * gate;
                buf_store(v, d_in, idx[row] >= 0 ? (unsigned)idx[row] * 4u : BUF_OOB, 0u);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// first layer, forward: a thread owns four consecutive frames of one row (signal, b); the K + 3 samples are read once, then every
// channel is four fma chains over k ascending from 0, + bias, leaky ReLU, stored as 16 bytes when T % 4 == 0 (then every row and
// channel line is 16-byte aligned), else as four dwords.  Memory-bound on the [2 B][C][T] store.
// ------------------------------------------------------------------------------------------
constexpr int WAVE_KMAX = SET_WAVE_CONV_KMAX;

__global__ void __launch_bounds__(256) wave_conv_fwd_kernel(const float *y, const float *y_hat, const float *w, const float *bias, float *out, int B,
                                                            int T, int C, int K, int pad, int quads, int act, float slope, int64_t units) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= units) return;
    const int row = (int)(unit / quads);
    const int h = (int)(unit - (int64_t)row * quads) * 4;
    const float *src = (row >= B ? y_hat + (int64_t)(row - B) * T : y + (int64_t)row * T);
    float xv[WAVE_KMAX + 3];
#pragma unroll
    for (int i = 0; i < WAVE_KMAX + 3; ++i) {
        const int n = h + i - pad;
        const bool ok = i < K + 3 && n >= 0 && n < T;
        const float v = src[ok ? n : 0];
        xv[i] = ok ? v : 0.0f;
    }
    const float sl = act ? slope : 1.0f;
    float *o = out + (int64_t)row * C * T + h;
    const bool vec = (T & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int c = 0; c < C; ++c) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < WAVE_KMAX; ++k) {
            if (k < K) {  // uniform
                const float wk = w[c * K + k];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = fmaf(wk, xv[k + u], acc[u]);
            }
        }
        const float bv = bias ? bias[c] : 0.0f;
        f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float t = acc[u] + bv;
            v[u] = t > 0.0f ? t : t * sl;
        }
        float *oc = o + (int64_t)c * T;
        if (vec) {
            *reinterpret_cast<f32x4 *>(oc) = v;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (h + u < T) oc[u] = v[u];
        }
    }
}

// first layer, backward: g_wav[b][n] = fma chain over c ascending, inside it k ascending, of w[c][k] dz[b][c][n + pad - k] (a tap whose
// frame is outside [0, T) adds an exact 0).  A thread owns one sample; dz is read along n.
__global__ void __launch_bounds__(256) wave_conv_bwd_kernel(const float *dz, const float *w, float *g_wav, int B, int T, int C, int K, int pad,
                                                            int64_t units) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= units) return;
    const int b = (int)(unit / T);
    const int n = (int)(unit - (int64_t)b * T);
    int hh[WAVE_KMAX];
    bool ok[WAVE_KMAX];
#pragma unroll
    for (int k = 0; k < WAVE_KMAX; ++k) {
        const int t = n + pad - k;
        ok[k] = k < K && t >= 0 && t < T;
        hh[k] = ok[k] ? t : 0;
    }
    const float *dr = dz + (int64_t)b * C * T;
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float *dc = dr + (int64_t)c * T;
#pragma unroll
        for (int k = 0; k < WAVE_KMAX; ++k) {
            if (k < K) {  // uniform
                const float v = dc[hh[k]];
                acc = fmaf(w[c * K + k], ok[k] ? v : 0.0f, acc);
            }
        }
    }
    g_wav[unit] = acc;
}

// ------------------------------------------------------------------------------------------
// AvgPool1d(4, 2, padding = 1), count_include_pad: out[j] = 0.25 (((x[2 j - 1] + x[2 j]) + x[2 j + 1]) + x[2 j + 2]), zeros outside.
// Transpose: sample i feeds the outputs lo = (i + 1) / 2 - 1 and hi = lo + 1 (each where it lies in [0, T_out)):
//   g_in[i] = add[i] + (0.25 g_out[lo] + 0.25 g_out[hi]), a missing term an exact 0, add optional.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) avgpool4s2_fwd_kernel(const float *x, float *out, int T, int T_out, int64_t units) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= units) return;
    const int64_t b = unit / T_out;
    const int j = (int)(unit - b * T_out);
    const float *xr = x + b * T;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int n = 2 * j - 1 + u;
        const bool ok = n >= 0 && n < T;
        const float t = xr[ok ? n : 0];
        v[u] = ok ? t : 0.0f;
    }
    out[unit] = 0.25f * (((v[0] + v[1]) + v[2]) + v[3]);
}

__global__ void __launch_bounds__(256) avgpool4s2_bwd_kernel(const float *g_out, const float *add, float *g_in, int T, int T_out, int64_t units) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= units) return;
    const int64_t b = unit / T;
    const int i = (int)(unit - b * T);
    const float *gr = g_out + b * T_out;
    const int lo = (i + 1) / 2 - 1, hi = lo + 1;
    const bool lok = lo >= 0 && lo < T_out, hok = hi < T_out;
    const float gl = gr[lok ? lo : 0], gh = gr[hok ? hi : 0];
    const float s = 0.25f * (lok ? gl : 0.0f) + 0.25f * (hok ? gh : 0.0f);
    const float av = add ? add[unit] : 0.0f;
    g_in[unit] = add ? av + s : s;
}

bool gconv_shape_ok(int R, int Cin, int Cout, int groups, int H_in, int K, int s, int pad) {
    return R > 0 && Cin > 0 && Cout > 0 && groups > 0 && Cin % groups == 0 && Cout % groups == 0 && H_in > 0 && K >= 1 && K <= GCONV_KMAX && s >= 1 &&
           s <= 4 && pad >= 0 && pad < K;
}
inline int gconv_out_len(int H_in, int K, int s, int pad) { return H_in + 2 * pad >= K ? (H_in + 2 * pad - K) / s + 1 : 0; }
constexpr int64_t SLICE_LIMIT = (int64_t)1 << 29;  // floats: one row's [C][H] slice is addressed with 32-bit byte offsets

// the block shape by the 32-row blocks of a group: one block of rows -> four waves along the frames (128), more -> 2 x 2 (64 frames,
// two row blocks per block; further row blocks go to further blocks, which stage the window again)
template <typename F> int by_rows(int RBn, F &&f) {
    if (RBn == 1) return f(ic<1>{}, ic<4>{});
    return f(ic<2>{}, ic<2>{});
}

}  // namespace

extern "C" int32_t set_gconv1d_out_len(int32_t H_in, int32_t K, int32_t s, int32_t pad) {
    if (!gconv_shape_ok(1, 1, 1, 1, H_in, K, s, pad))
        return set_fail(SET_E_INVALID, "set_gconv1d_out_len", "needs H_in > 0, 1 <= K <= 41, 1 <= s <= 4, 0 <= pad < K");
    return gconv_out_len(H_in, K, s, pad);
}

extern "C" int32_t set_gconv1d_tile(int32_t rows_per_group) {
    if (rows_per_group <= 0) return set_fail(SET_E_INVALID, "set_gconv1d_tile", "needs rows_per_group > 0");
    const int RBn = (rows_per_group + 31) / 32;
    return RBn == 1 ? SET_GCONV_TILE_1 : SET_GCONV_TILE_2;
}

extern "C" int64_t set_packed_gconv_weight_size(int32_t Cout, int32_t Cin, int32_t K, int32_t groups) {
    if (Cout <= 0 || Cin <= 0 || K <= 0 || groups <= 0 || Cout % groups || Cin % groups)
        return set_fail(SET_E_INVALID, "set_packed_gconv_weight_size", "groups must divide Cin and Cout");
    return (int64_t)groups * set_packed_conv_weight_size(Cout / groups, Cin / groups, K);
}

extern "C" int set_gconv1d_fwd(const float *x, const float *wp, const float *bias, float *out, int32_t R, int32_t Cin, int32_t Cout, int32_t groups,
                               int32_t H_in, int32_t K, int32_t s, int32_t pad, int32_t act, float slope, void *stream) {
    SET_REQUIRE(x && wp && out, "set_gconv1d_fwd");
    SET_REQUIRE(gconv_shape_ok(R, Cin, Cout, groups, H_in, K, s, pad), "set_gconv1d_fwd");
    SET_REQUIRE(act == 0 || act == 1, "set_gconv1d_fwd");
    const int H_out = gconv_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, "set_gconv1d_fwd");
    if ((int64_t)Cin * H_in >= SLICE_LIMIT || (int64_t)Cout * H_out >= SLICE_LIMIT)
        return set_fail(SET_E_UNSUPPORTED, "set_gconv1d_fwd", "one row's [C][H] slice exceeds 2 GiB");
    const int Cin_g = Cin / groups, Cout_g = Cout / groups;
    const int CinP = set_round_up(Cin_g, KC), RBn = (Cout_g + 31) / 32;
    GconvArgs a{x, wp, bias, out, R, Cin_g, Cout_g, groups, H_in, H_out, K, pad, act, slope};
    auto launch = [&](auto S_, auto WM_, auto WN_) {
        constexpr int S = decltype(S_)::value, WM = decltype(WM_)::value, WN = decltype(WN_)::value, BN = 32 * WN;
        const int tiles = (H_out + BN - 1) / BN, RBY = (RBn + WM - 1) / WM;
        if ((int64_t)R * tiles > 0x7fffffff || (int64_t)groups * RBY > 65535)
            return set_fail(SET_E_UNSUPPORTED, "set_gconv1d_fwd", "more than 2^31 - 1 tiles or 65535 row blocks");
        const size_t lds = (size_t)KC * S * (BN + (K - 1) / S) * sizeof(float);  // <= 35 KiB
        hipLaunchKernelGGL((gconv1d_fwd_kernel<S, WM, WN>), dim3((unsigned)(R * tiles), groups * RBY), dim3(256), lds, (hipStream_t)stream, a, CinP, RBn,
                           RBY, tiles);
        return set_check_launch("set_gconv1d_fwd");
    };
    auto shape = [&](auto S_) { return by_rows(RBn, [&](auto WM_, auto WN_) { return launch(S_, WM_, WN_); }); };
    if (s == 1) return shape(ic<1>{});
    if (s == 2) return shape(ic<2>{});
    if (s == 3) return shape(ic<3>{});
    return shape(ic<4>{});
}

extern "C" int set_gconv1d_dgrad(const float *dz_out, const float *wtp, const float *f_in, const float *add, float *dz_in, int32_t R, int32_t Cin,
                                 int32_t Cout, int32_t groups, int32_t H_in, int32_t K, int32_t s, int32_t pad, float slope, void *stream) {
    SET_REQUIRE(dz_out && wtp && dz_in, "set_gconv1d_dgrad");
    SET_REQUIRE(gconv_shape_ok(R, Cin, Cout, groups, H_in, K, s, pad), "set_gconv1d_dgrad");
    const int H_out = gconv_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, "set_gconv1d_dgrad");
    if ((int64_t)Cin * H_in >= SLICE_LIMIT || (int64_t)Cout * H_out >= SLICE_LIMIT)
        return set_fail(SET_E_UNSUPPORTED, "set_gconv1d_dgrad", "one row's [C][H] slice exceeds 2 GiB");
    const int Cin_g = Cin / groups, Cout_g = Cout / groups;
    const int CoP = set_round_up(Cout_g, KC), RBn = (Cin_g + 31) / 32;
    GdgradArgs a{dz_out, wtp, f_in, add, dz_in, R, Cin_g, Cout_g, groups, H_in, H_out, K, pad, slope};
    auto launch = [&](auto S_, auto WM_, auto WN_) {
        constexpr int S = decltype(S_)::value, WM = decltype(WM_)::value, WN = decltype(WN_)::value, JW = S * 32 * WN;
        const int tiles = (H_in + JW - 1) / JW, RBY = (RBn + WM - 1) / WM;
        if ((int64_t)R * tiles > 0x7fffffff || (int64_t)groups * RBY > 65535)
            return set_fail(SET_E_UNSUPPORTED, "set_gconv1d_dgrad", "more than 2^31 - 1 tiles or 65535 row blocks");
        const size_t stage = (size_t)KC * (32 * WN + (K - 1) / S + (S - 1 + pad) / S) * sizeof(float), epi = (size_t)4 * 8 * S * 32 * sizeof(float);
        hipLaunchKernelGGL((gconv1d_dgrad_kernel<S, WM, WN>), dim3((unsigned)(R * tiles), groups * RBY), dim3(256), stage > epi ? stage : epi,
                           (hipStream_t)stream, a, CoP, RBn, RBY, tiles);
        return set_check_launch("set_gconv1d_dgrad");
    };
    auto shape = [&](auto S_) { return by_rows(RBn, [&](auto WM_, auto WN_) { return launch(S_, WM_, WN_); }); };
    if (s == 1) return shape(ic<1>{});
    if (s == 2) return shape(ic<2>{});
    if (s == 3) return shape(ic<3>{});
    return shape(ic<4>{});
}

static bool wave_shape_ok(int B, int T, int C, int K, int pad) {
    return B > 0 && T > 0 && T <= (1 << 30) && C > 0 && K >= 1 && K <= WAVE_KMAX && pad >= 0 && pad < K && T + 2 * pad - K + 1 == T;
}

extern "C" int set_wave_conv_fwd(const float *y, const float *y_hat, const float *w, const float *bias, float *out, int32_t B, int32_t T, int32_t C,
                                 int32_t K, int32_t pad, int32_t act, float slope, void *stream) {
    SET_REQUIRE(y && w && out, "set_wave_conv_fwd");
    SET_REQUIRE(wave_shape_ok(B, T, C, K, pad), "set_wave_conv_fwd");
    SET_REQUIRE(act == 0 || act == 1, "set_wave_conv_fwd");
    const int quads = (T + 3) / 4;
    const int64_t units = (int64_t)(y_hat ? 2 : 1) * B * quads;  // y_hat NULL: the B rows of y alone
    if ((units + 255) / 256 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_wave_conv_fwd", "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(wave_conv_fwd_kernel, dim3(set_blocks(units, 256)), dim3(256), 0, (hipStream_t)stream, y, y_hat, w, bias, out, B, T, C, K, pad, quads,
                       act, slope, units);
    return set_check_launch("set_wave_conv_fwd");
}

extern "C" int set_wave_conv_bwd(const float *dz, const float *w, float *g_wav, int32_t B, int32_t T, int32_t C, int32_t K, int32_t pad, void *stream) {
    SET_REQUIRE(dz && w && g_wav, "set_wave_conv_bwd");
    SET_REQUIRE(wave_shape_ok(B, T, C, K, pad), "set_wave_conv_bwd");
    const int64_t units = (int64_t)B * T;
    if ((units + 255) / 256 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_wave_conv_bwd", "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(wave_conv_bwd_kernel, dim3(set_blocks(units, 256)), dim3(256), 0, (hipStream_t)stream, dz, w, g_wav, B, T, C, K, pad, units);
    return set_check_launch("set_wave_conv_bwd");
}

extern "C" int32_t set_avgpool4s2_out_len(int32_t T) { return T >= 2 ? (T - 2) / 2 + 1 : 0; }

extern "C" int set_avgpool4s2_fwd(const float *x, float *out, int32_t B, int32_t T, void *stream) {
    SET_REQUIRE(x && out && B > 0 && T >= 2, "set_avgpool4s2_fwd");
    const int T_out = set_avgpool4s2_out_len(T);
    const int64_t units = (int64_t)B * T_out;
    if ((units + 255) / 256 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_avgpool4s2_fwd", "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(avgpool4s2_fwd_kernel, dim3(set_blocks(units, 256)), dim3(256), 0, (hipStream_t)stream, x, out, T, T_out, units);
    return set_check_launch("set_avgpool4s2_fwd");
}

extern "C" int set_avgpool4s2_bwd(const float *g_out, const float *add, float *g_in, int32_t B, int32_t T, void *stream) {
    SET_REQUIRE(g_out && g_in && B > 0 && T >= 2, "set_avgpool4s2_bwd");
    const int T_out = set_avgpool4s2_out_len(T);
    const int64_t units = (int64_t)B * T;
    if ((units + 255) / 256 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, "set_avgpool4s2_bwd", "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(avgpool4s2_bwd_kernel, dim3(set_blocks(units, 256)), dim3(256), 0, (hipStream_t)stream, g_out, add, g_in, T, T_out, units);
    return set_check_launch("set_avgpool4s2_bwd");
}
