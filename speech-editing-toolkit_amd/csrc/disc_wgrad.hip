// The discriminator step of HiFi-GAN (tasks/vocoder/hifigan.py:51-61): the gradients with respect to the discriminators' own weights.
//   gconv1d_wgrad_kernel      weight gradient of the grouped / dense strided 1-D convolutions of sconv.hip and msd.hip, an implicit GEMM
//                             on v_mfma_f32_32x32x2_f32 whose reduction index runs over the frames of ALL rows, cut into slices
//   wgrad_reduce_kernel       the ordered sum of the slices' partials (and the add into dW)
//   channel_sum_rows_kernel   the bias gradient of those layers
//   first_wgrad_*_kernel      weight and bias gradient of the two first layers (one input channel), straight from the waveforms
//   wn_fold_bwd_kernel, sn_fold_bwd_*_kernel   the backward of the weight-norm and the spectral-norm fold
// Activations are [R][C][H] rows as in sconv.hip.  No atomics: every sum has one documented order (include/set_amd.h).
#include "common.h"

namespace {

constexpr int WG_CH = SET_GCONV_WGRAD_CHUNK;  // reduction indices of one chunk
constexpr int WG_COLS = SET_GCONV_WGRAD_COLS;  // flattened (ci, k) columns of one block: 32 per wave
constexpr int A_LD = WG_CH + 1, B_LD = WG_COLS + 1;
constexpr int A_PER = WG_CH * 32 / 256, B_PER = WG_CH * WG_COLS / 256;
static_assert(WG_CH == 32 && WG_COLS == 128, "the staging below maps 256 threads to 32 reduction indices x 8 lines");

struct WgradArgs {
    const float *dz, *x;
    float *part;
    int Cin_g, Cout_g, groups, H_in, H_out, K, s, pad;
    int J, nchunks, cps, N, MB;
    int64_t slice_stride;
};

// ------------------------------------------------------------------------------------------
// dW_g [Cout / G][(ci, k)] = dz_g [Cout / G][j] . X_g [j][(ci, k)],  j = r H_out + h over the frames of every row,
// X_g[j][(ci, k)] = x[r][g Cin/G + ci][s h + k - pad] (0 outside the row).  block = 4 waves: one 32-row block of one group by 128
// flattened (ci, k) columns (32 per wave, one 32x32 accumulator each), over the chunks of 32 reduction indices of one slice.
// A chunk is staged as As[j][co] (line stride 33) and Bs[j][col] (line stride 129): thread (jj = tid % 32, q = tid / 32) gathers
// reduction index jj of lines q, q + 8, ..  The 32 lanes of a half-wave share q, so their LDS writes go to banks (jj + line) % 32:
// conflict-free; their global reads run along h at stride s (x) or 1 (dz).  The MFMA operand reads are lane-consecutive dwords of one
// line.  None of this depends on s or on where a row ends: the stride and the row only enter the gather address, so a chunk holds the
// frames of as many rows as fall into it and ragged Cin / G costs nothing but the last column block's padding.
// The next chunk's gather is issued before the current chunk's MFMAs and lands in LDS after them.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gconv1d_wgrad_kernel(WgradArgs a) {
    __shared__ float As[WG_CH * A_LD];
    __shared__ float Bs[WG_CH * B_LD];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int jj = tid & 31, q = tid >> 5;
    const int cb = blockIdx.x;
    const int g = blockIdx.y / a.MB, mb = blockIdx.y - g * a.MB;
    const int sl = blockIdx.z;
    const int c_first = sl * a.cps, c_last = min(c_first + a.cps, a.nchunks);
    const int Cin = a.Cin_g * a.groups, Cout = a.Cout_g * a.groups;

    int a_off[A_PER];  // (channel of dz) H_out, or -1
#pragma unroll
    for (int u = 0; u < A_PER; ++u) {
        const int co = mb * 32 + q + 8 * u;
        a_off[u] = co < a.Cout_g ? (g * a.Cout_g + co) * a.H_out : -1;
    }
    int b_off[B_PER], b_k[B_PER];  // (channel of x) H_in + k - pad, and k - pad; column past N: b_k = INT_MIN / 2 (never in range)
#pragma unroll
    for (int u = 0; u < B_PER; ++u) {
        const int col = cb * WG_COLS + q + 8 * u;
        const bool ok = col < a.N;
        const int ci = ok ? col / a.K : 0, k = ok ? col - ci * a.K : 0;
        b_k[u] = ok ? k - a.pad : -(1 << 30);
        b_off[u] = (g * a.Cin_g + ci) * a.H_in + k - a.pad;
    }
    float av[A_PER], bv[B_PER];
    auto gather = [&](int c) __attribute__((always_inline)) {
        const int j = c * WG_CH + jj;
        const bool jv = j < a.J;
        const int r = jv ? j / a.H_out : 0;
        const int h = jv ? j - r * a.H_out : 0;
        const float *dr = a.dz + (int64_t)r * Cout * a.H_out + h;
        const float *xr = a.x + (int64_t)r * Cin * a.H_in + a.s * h;
#pragma unroll
        for (int u = 0; u < A_PER; ++u) {
            const bool ok = jv && a_off[u] >= 0;
            const float v = dr[ok ? a_off[u] : -h];
            av[u] = ok ? v : 0.0f;
        }
        const int p0 = a.s * h;
#pragma unroll
        for (int u = 0; u < B_PER; ++u) {
            const int p = p0 + b_k[u];
            const bool ok = jv && p >= 0 && p < a.H_in;
            const float v = xr[ok ? b_off[u] : -p0];
            bv[u] = ok ? v : 0.0f;
        }
    };

    f32x16 acc = (f32x16){0};
    const bool cols_live = cb * WG_COLS + wave * 32 < a.N;
    if (c_first < c_last) gather(c_first);
    for (int c = c_first; c < c_last; ++c) {
        __syncthreads();  // the previous chunk is consumed
#pragma unroll
        for (int u = 0; u < A_PER; ++u) As[jj * A_LD + q + 8 * u] = av[u];
#pragma unroll
        for (int u = 0; u < B_PER; ++u) Bs[jj * B_LD + q + 8 * u] = bv[u];
        __syncthreads();
        if (c + 1 < c_last) gather(c + 1);
        if (cols_live) {
            const float *ap = As + half * A_LD + l31;
            const float *bp = Bs + half * B_LD + wave * 32 + l31;
#pragma unroll
            for (int st = 0; st < WG_CH / 2; ++st) acc = mfma32(ap[2 * st * A_LD], bp[2 * st * B_LD], acc);
        }
    }
    if (!cols_live) return;
    const int col = cb * WG_COLS + wave * 32 + l31;
    float *o = a.part + (int64_t)sl * a.slice_stride + (int64_t)(g * a.Cout_g) * a.N + col;
#pragma unroll
    for (int qr = 0; qr < 16; ++qr) {
        const int co = mb * 32 + 4 * half + urow16(qr);
        if (co < a.Cout_g && col < a.N) o[(int64_t)co * a.N] = acc[qr];
    }
}

// dW[e] = (accumulate ? dW[e] : nothing) + ((part[0][e] + part[1][e]) + ..): the slices in ascending order, then the old value
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float *part, float *dw, int64_t n, int slices, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float t = part[e];
    for (int z = 1; z < slices; ++z) t += part[(int64_t)z * n + e];
    dw[e] = accumulate ? dw[e] + t : t;
}

// the 256 thread sums of a block, halved: red[t] += red[t + st], st = 128, 64, .. 1; every thread returns red[0]
__device__ __forceinline__ double block_sum(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st) red[t] += red[t + st];
        __syncthreads();
    }
    return red[0];
}

// db[c] = sum over (r, h) of dz[r][c][h]: block c; thread t adds the elements j = t, t + 256, .. (j = r H + h) in double, then block_sum
__global__ void __launch_bounds__(256) channel_sum_rows_kernel(const float *dz, float *db, int C, int H, int64_t J, int accumulate) {
    __shared__ double red[256];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < J; j += 256) {
        const int64_t r = j / H;
        s += (double)dz[(r * C + c) * H + (j - r * H)];
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) db[c] = accumulate ? db[c] + (float)tot : (float)tot;
}

// ------------------------------------------------------------------------------------------
// first layers: dW[c][k] = sum_j dz[r][c][h] X(r, s h + k - pad), db[c] = sum_j dz[r][c][h], j = r H_out + h over all rows.
// Block (c, slice): thread t adds the terms of j = lo + t, lo + t + 256, .. below hi (the slice's range) in double, products exact;
// block_sum per tap -> part[slice][c][k] (k = K: the bias slot).  The finish adds the slices in ascending order in double.
// FOLD: X is the MPD's folded, mirror-padded waveform (row (sig B + b) p + w reads xpad[i p + w]); else the MSD's plain one.
// ------------------------------------------------------------------------------------------
constexpr int FIRST_KMAX = SET_WAVE_CONV_KMAX;

struct FirstArgs {
    const float *dz, *y, *y_hat;
    double *part;
    int B, T, p, C, K, s, pad, H, H_out;
    int64_t J, per;
};

template <bool FOLD>
__global__ void __launch_bounds__(256) first_wgrad_part_kernel(FirstArgs a) {
    __shared__ double red[256];
    const int c = blockIdx.x, sl = blockIdx.y;
    const int64_t lo = (int64_t)sl * a.per, hi = min(lo + a.per, a.J);
    double acc[FIRST_KMAX + 1];
#pragma unroll
    for (int k = 0; k <= FIRST_KMAX; ++k) acc[k] = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const int r = (int)(j / a.H_out);
        const int h = (int)(j - (int64_t)r * a.H_out);
        const double d = (double)a.dz[((int64_t)r * a.C + c) * a.H_out + h];
        int sigb, w;
        if constexpr (FOLD) {
            sigb = r / a.p;
            w = r - sigb * a.p;
        } else {
            sigb = r;
            w = 0;
        }
        const float *src = sigb >= a.B ? a.y_hat + (int64_t)(sigb - a.B) * a.T : a.y + (int64_t)sigb * a.T;
#pragma unroll
        for (int k = 0; k < FIRST_KMAX; ++k) {
            if (k < a.K) {  // uniform
                const int i = a.s * h + k - a.pad;
                const bool ok = i >= 0 && i < a.H;
                int n = ok ? (FOLD ? i * a.p + w : i) : 0;
                if (FOLD && n >= a.T) n = 2 * (a.T - 1) - n;
                const float v = src[n];
                acc[k] += d * (double)(ok ? v : 0.0f);
            }
        }
        acc[FIRST_KMAX] += d;
    }
    double *o = a.part + ((int64_t)sl * a.C + c) * (a.K + 1);
#pragma unroll
    for (int k = 0; k < FIRST_KMAX; ++k) {
        if (k < a.K) {
            const double t = block_sum(acc[k], red);
            if (threadIdx.x == 0) o[k] = t;
        }
    }
    const double tb = block_sum(acc[FIRST_KMAX], red);
    if (threadIdx.x == 0) o[a.K] = tb;
}

__global__ void __launch_bounds__(256) first_wgrad_finish_kernel(const double *part, float *dw, float *db, int C, int K, int slices, int accumulate) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * (K + 1)) return;
    const int c = e / (K + 1), k = e - c * (K + 1);
    double t = part[e];
    for (int z = 1; z < slices; ++z) t += part[(int64_t)z * C * (K + 1) + e];
    float *o = k < K ? (dw ? dw + c * K + k : nullptr) : (db ? db + c : nullptr);
    if (o) *o = accumulate ? *o + (float)t : (float)t;
}

// ------------------------------------------------------------------------------------------
// weight-norm fold backward, one block per row: thread t adds v[i]^2 and dW[i] v[i] of i = t, t + 256, .. in double, block_sum each;
// n = sqrt(sum v^2);  dg = <dW, v> / n;  dv[i] = (g / n) (dW[i] - v[i] <dW, v> / n^2), all in double, rounded once.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wn_fold_bwd_kernel(const float *dw, const float *g, const float *v, float *dg, float *dv, int64_t inner,
                                                          int accumulate) {
    __shared__ double red[256];
    const int64_t base = (int64_t)blockIdx.x * inner;
    double sv = 0.0, sd = 0.0;
    for (int64_t i = threadIdx.x; i < inner; i += 256) {
        const double vi = (double)v[base + i];
        sv += vi * vi;
        sd += (double)dw[base + i] * vi;
    }
    const double n2 = block_sum(sv, red);
    const double dot = block_sum(sd, red);
    const double n = sqrt(n2);
    if (dg && threadIdx.x == 0) {
        const float r = (float)(dot / n);
        dg[blockIdx.x] = accumulate ? dg[blockIdx.x] + r : r;
    }
    if (!dv) return;
    const double gn = (double)g[blockIdx.x] / n, pr = dot / n2;
    for (int64_t i = threadIdx.x; i < inner; i += 256) {
        const float r = (float)(gn * ((double)dw[base + i] - (double)v[base + i] * pr));
        dv[base + i] = accumulate ? dv[base + i] + r : r;
    }
}

// spectral-norm fold backward.  Pass 1, one block per row: part[row] = sum_i dW[row][i] W[row][i] as above.  Pass 2: every block adds
// the row sums (thread t: rows t, t + 256, .. ascending; block_sum) to the same total, then
// d W_orig[e] = (dW[e] - (total / sigma) u[row] v[i]) / sigma in double, rounded once.
__global__ void __launch_bounds__(256) sn_fold_bwd_rows_kernel(const float *dw, const float *w, double *part, int64_t inner) {
    __shared__ double red[256];
    const int64_t base = (int64_t)blockIdx.x * inner;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < inner; i += 256) s += (double)dw[base + i] * (double)w[base + i];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) sn_fold_bwd_apply_kernel(const float *dw, const float *u, const float *v, const float *sigma, const double *part,
                                                                float *dw_orig, int n0, int64_t inner, int64_t n, int accumulate) {
    __shared__ double red[256];
    double s = 0.0;
    for (int r = threadIdx.x; r < n0; r += 256) s += part[r];
    const double tot = block_sum(s, red);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t row = e / inner, i = e - row * inner;
    const double sg = (double)sigma[0];
    const float r = (float)(((double)dw[e] - (tot / sg) * (double)u[row] * (double)v[i]) / sg);
    dw_orig[e] = accumulate ? dw_orig[e] + r : r;
}

bool wgrad_shape_ok(int R, int Cin, int Cout, int groups, int H_in, int K, int s, int pad) {
    return R > 0 && Cin > 0 && Cout > 0 && groups > 0 && Cin % groups == 0 && Cout % groups == 0 && H_in > 0 && K >= 1 && K <= SET_GCONV_KMAX && s >= 1 &&
           s <= 4 && pad >= 0 && pad < K;
}
inline int wgrad_out_len(int H_in, int K, int s, int pad) { return H_in + 2 * pad >= K ? (H_in + 2 * pad - K) / s + 1 : 0; }
constexpr int64_t SLICE_LIMIT = (int64_t)1 << 29;

// the number of reduction slices: enough blocks for four per CU, no slice shorter than 8 chunks, at most SET_GCONV_WGRAD_MAX_SLICES
int wgrad_plan(int64_t J, int Cin_g, int Cout_g, int groups, int K, int n_cu) {
    const int64_t nchunks = (J + WG_CH - 1) / WG_CH;
    const int64_t tiles = (int64_t)groups * ((Cout_g + 31) / 32) * (((int64_t)Cin_g * K + WG_COLS - 1) / WG_COLS);
    int64_t want = (4 * (int64_t)n_cu + tiles - 1) / tiles;
    const int64_t cap = nchunks / 8;
    if (want > cap) want = cap;
    if (want > SET_GCONV_WGRAD_MAX_SLICES) want = SET_GCONV_WGRAD_MAX_SLICES;
    return want < 1 ? 1 : (int)want;
}

int resolve_cu(int n_cu, const char *what) {
    if (n_cu > 0) return n_cu;
    int n = 0;
    const hipError_t e = set_cu_count(&n);
    if (e != hipSuccess) return set_fail(SET_E_LAUNCH, what, hipGetErrorString(e));
    return n;
}

int first_plan(int64_t J, int C, int n_cu) {
    int64_t want = (4 * (int64_t)n_cu + C - 1) / C;
    const int64_t cap = J / 4096;  // no slice below 16 terms per thread
    if (want > cap) want = cap;
    if (want > SET_FIRST_WGRAD_MAX_SLICES) want = SET_FIRST_WGRAD_MAX_SLICES;
    return want < 1 ? 1 : (int)want;
}

int first_launch(bool fold, FirstArgs a, float *dw, float *db, int accumulate, int slices, int64_t part_doubles, void *stream, const char *what) {
    if (slices < 0 || slices > SET_FIRST_WGRAD_MAX_SLICES) return set_fail(SET_E_INVALID, what, "slices must be 0 (the plan's) .. SET_FIRST_WGRAD_MAX_SLICES");
    if (slices == 0) {
        const int n_cu = resolve_cu(0, what);
        if (n_cu < 0) return n_cu;
        slices = first_plan(a.J, a.C, n_cu);
    }
    if (part_doubles < (int64_t)slices * a.C * (a.K + 1)) return set_fail(SET_E_INVALID, what, "part is too small");
    a.per = (a.J + slices - 1) / slices;
    if (fold)
        hipLaunchKernelGGL(first_wgrad_part_kernel<true>, dim3(a.C, slices), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(first_wgrad_part_kernel<false>, dim3(a.C, slices), dim3(256), 0, (hipStream_t)stream, a);
    int rc = set_check_launch(what);
    if (rc != SET_OK) return rc;
    hipLaunchKernelGGL(first_wgrad_finish_kernel, dim3(set_blocks((int64_t)a.C * (a.K + 1), 256)), dim3(256), 0, (hipStream_t)stream, a.part, dw, db, a.C, a.K,
                       slices, accumulate);
    return set_check_launch(what);
}

}  // namespace

extern "C" int32_t set_gconv1d_wgrad_plan(int32_t R, int32_t Cin, int32_t Cout, int32_t groups, int32_t H_in, int32_t K, int32_t s, int32_t pad,
                                          int32_t n_cu) {
    if (!wgrad_shape_ok(R, Cin, Cout, groups, H_in, K, s, pad) || n_cu < 0)
        return set_fail(SET_E_INVALID, "set_gconv1d_wgrad_plan", "needs the ranges of set_gconv1d_fwd and n_cu >= 0");
    const int H_out = wgrad_out_len(H_in, K, s, pad);
    if (H_out < 1) return set_fail(SET_E_INVALID, "set_gconv1d_wgrad_plan", "no output frame");
    n_cu = resolve_cu(n_cu, "set_gconv1d_wgrad_plan");
    if (n_cu < 0) return n_cu;
    return wgrad_plan((int64_t)R * H_out, Cin / groups, Cout / groups, groups, K, n_cu);
}

extern "C" int64_t set_gconv1d_wgrad_scratch_floats(int32_t R, int32_t Cin, int32_t Cout, int32_t groups, int32_t H_in, int32_t K, int32_t s, int32_t pad,
                                                    int32_t slices) {
    if (slices < 0 || slices > SET_GCONV_WGRAD_MAX_SLICES)
        return set_fail(SET_E_INVALID, "set_gconv1d_wgrad_scratch_floats", "slices must be 0 (the plan's) .. SET_GCONV_WGRAD_MAX_SLICES");
    if (slices == 0) {
        slices = set_gconv1d_wgrad_plan(R, Cin, Cout, groups, H_in, K, s, pad, 0);
        if (slices < 0) return slices;
    } else if (!wgrad_shape_ok(R, Cin, Cout, groups, H_in, K, s, pad)) {
        return set_fail(SET_E_INVALID, "set_gconv1d_wgrad_scratch_floats", "needs the ranges of set_gconv1d_fwd");
    }
    return (int64_t)slices * Cout * (Cin / groups) * K;
}

extern "C" int set_gconv1d_wgrad(const float *dz, const float *x, float *dw, float *db, int32_t R, int32_t Cin, int32_t Cout, int32_t groups, int32_t H_in,
                                 int32_t K, int32_t s, int32_t pad, int32_t accumulate, int32_t slices, float *scratch, int64_t scratch_floats,
                                 void *stream) {
    const char *what = "set_gconv1d_wgrad";
    SET_REQUIRE(dz && x && (dw || db), what);
    SET_REQUIRE(wgrad_shape_ok(R, Cin, Cout, groups, H_in, K, s, pad), what);
    SET_REQUIRE(accumulate == 0 || accumulate == 1, what);
    SET_REQUIRE(slices >= 0 && slices <= SET_GCONV_WGRAD_MAX_SLICES, what);
    const int H_out = wgrad_out_len(H_in, K, s, pad);
    SET_REQUIRE(H_out > 0, what);
    if ((int64_t)Cin * H_in >= SLICE_LIMIT || (int64_t)Cout * H_out >= SLICE_LIMIT)
        return set_fail(SET_E_UNSUPPORTED, what, "one row's [C][H] slice exceeds 2 GiB");
    const int64_t J = (int64_t)R * H_out;
    if (J > 0x7fffffff - WG_CH) return set_fail(SET_E_UNSUPPORTED, what, "more than 2^31 - 1 frames over all rows");
    const int Cin_g = Cin / groups, Cout_g = Cout / groups;
    if (dw) {
        if (slices == 0) {
            const int n_cu = resolve_cu(0, what);
            if (n_cu < 0) return n_cu;
            slices = wgrad_plan(J, Cin_g, Cout_g, groups, K, n_cu);
        }
        const int64_t n = (int64_t)Cout * Cin_g * K;
        const bool direct = slices == 1 && !accumulate;  // the one slice's plain stores are the result
        if (!direct) {
            SET_REQUIRE(scratch != nullptr, what);
            if (scratch_floats < slices * n) return set_fail(SET_E_INVALID, what, "scratch is too small (set_gconv1d_wgrad_scratch_floats)");
        }
        WgradArgs a;
        a.dz = dz, a.x = x, a.part = direct ? dw : scratch;
        a.Cin_g = Cin_g, a.Cout_g = Cout_g, a.groups = groups, a.H_in = H_in, a.H_out = H_out, a.K = K, a.s = s, a.pad = pad;
        a.J = (int)J, a.nchunks = (int)((J + WG_CH - 1) / WG_CH), a.cps = (a.nchunks + slices - 1) / slices;
        a.N = Cin_g * K, a.MB = (Cout_g + 31) / 32, a.slice_stride = n;
        const int ncb = (a.N + WG_COLS - 1) / WG_COLS;
        if ((int64_t)groups * a.MB > 65535) return set_fail(SET_E_UNSUPPORTED, what, "more than 65535 row blocks");
        hipLaunchKernelGGL(gconv1d_wgrad_kernel, dim3(ncb, groups * a.MB, slices), dim3(256), 0, (hipStream_t)stream, a);
        int rc = set_check_launch(what);
        if (rc != SET_OK) return rc;
        if (!direct) {
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(set_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, scratch, dw, n, slices, accumulate);
            rc = set_check_launch(what);
            if (rc != SET_OK) return rc;
        }
    }
    if (db) {
        hipLaunchKernelGGL(channel_sum_rows_kernel, dim3(Cout), dim3(256), 0, (hipStream_t)stream, dz, db, Cout, H_out, J, accumulate);
        return set_check_launch(what);
    }
    return SET_OK;
}

extern "C" int64_t set_first_conv_wgrad_part_doubles(int32_t C, int32_t K, int32_t slices) {
    if (C <= 0 || K < 1 || K > FIRST_KMAX || slices < 0 || slices > SET_FIRST_WGRAD_MAX_SLICES)
        return set_fail(SET_E_INVALID, "set_first_conv_wgrad_part_doubles", "needs C > 0, 1 <= K <= 15, 0 <= slices <= SET_FIRST_WGRAD_MAX_SLICES");
    return (int64_t)(slices ? slices : SET_FIRST_WGRAD_MAX_SLICES) * C * (K + 1);
}

extern "C" int set_mpd_fold_conv_wgrad(const float *dz, const float *y, const float *y_hat, float *dw, float *db, int32_t B, int32_t T, int32_t p,
                                       int32_t C, int32_t K, int32_t s, int32_t pad, int32_t accumulate, int32_t slices, double *part,
                                       int64_t part_doubles, void *stream) {
    const char *what = "set_mpd_fold_conv_wgrad";
    SET_REQUIRE(dz && y && y_hat && (dw || db) && part, what);
    SET_REQUIRE(B > 0 && p >= 1 && T > p && T <= (1 << 30) && C > 0 && K >= 1 && K <= FIRST_KMAX && s >= 1 && s <= 4 && pad >= 0 && pad < K, what);
    SET_REQUIRE(accumulate == 0 || accumulate == 1, what);
    const int H = (T + p - 1) / p;
    const int H_out = wgrad_out_len(H, K, s, pad);
    SET_REQUIRE(H_out > 0, what);
    if ((int64_t)C * H_out >= SLICE_LIMIT || (int64_t)2 * B * p > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, what, "one row's [C][H] slice exceeds 2 GiB");
    FirstArgs a{dz, y, y_hat, part, B, T, p, C, K, s, pad, H, H_out, (int64_t)2 * B * p * H_out, 0};
    return first_launch(true, a, dw, db, accumulate, slices, part_doubles, stream, what);
}

extern "C" int set_wave_conv_wgrad(const float *dz, const float *y, const float *y_hat, float *dw, float *db, int32_t B, int32_t T, int32_t C, int32_t K,
                                   int32_t pad, int32_t accumulate, int32_t slices, double *part, int64_t part_doubles, void *stream) {
    const char *what = "set_wave_conv_wgrad";
    SET_REQUIRE(dz && y && (dw || db) && part, what);
    SET_REQUIRE(B > 0 && T > 0 && T <= (1 << 30) && C > 0 && K >= 1 && K <= FIRST_KMAX && pad >= 0 && pad < K && T + 2 * pad - K + 1 == T, what);
    SET_REQUIRE(accumulate == 0 || accumulate == 1, what);
    if ((int64_t)C * T >= SLICE_LIMIT) return set_fail(SET_E_UNSUPPORTED, what, "one row's [C][H] slice exceeds 2 GiB");
    const int rows = (y_hat ? 2 : 1) * B;  // y_hat NULL: the B rows of y alone (a spectrally normed net in train() runs one signal at a time)
    FirstArgs a{dz, y, y_hat ? y_hat : y, part, B, T, 1, C, K, 1, pad, T, T, (int64_t)rows * T, 0};
    return first_launch(false, a, dw, db, accumulate, slices, part_doubles, stream, what);
}

extern "C" int set_weight_norm_fold_bwd(const float *dw, const float *g, const float *v, float *dg, float *dv, int32_t n0, int64_t inner,
                                        int32_t accumulate, void *stream) {
    const char *what = "set_weight_norm_fold_bwd";
    SET_REQUIRE(dw && g && v && (dg || dv), what);
    SET_REQUIRE(n0 > 0 && inner > 0 && (accumulate == 0 || accumulate == 1), what);
    hipLaunchKernelGGL(wn_fold_bwd_kernel, dim3(n0), dim3(256), 0, (hipStream_t)stream, dw, g, v, dg, dv, inner, accumulate);
    return set_check_launch(what);
}

extern "C" int set_spectral_norm_fold_bwd(const float *dw, const float *w_orig, const float *u, const float *v, const float *sigma, float *dw_orig,
                                          int32_t n0, int64_t inner, int32_t accumulate, double *part, void *stream) {
    const char *what = "set_spectral_norm_fold_bwd";
    SET_REQUIRE(dw && w_orig && u && v && sigma && dw_orig && part, what);
    SET_REQUIRE(n0 > 0 && inner > 0 && (accumulate == 0 || accumulate == 1), what);
    const int64_t n = (int64_t)n0 * inner;
    if ((n + 255) / 256 > 0x7fffffff) return set_fail(SET_E_UNSUPPORTED, what, "more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(sn_fold_bwd_rows_kernel, dim3(n0), dim3(256), 0, (hipStream_t)stream, dw, w_orig, part, inner);
    int rc = set_check_launch(what);
    if (rc != SET_OK) return rc;
    hipLaunchKernelGGL(sn_fold_bwd_apply_kernel, dim3(set_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, dw, u, v, sigma, part, dw_orig, n0, inner, n,
                       accumulate);
    return set_check_launch(what);
}
