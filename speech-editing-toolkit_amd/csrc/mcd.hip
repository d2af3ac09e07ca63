// Mel-cepstral distortion on the device (utils/eval/mcd.py `get_metrics_mels`): mel -> MFCC -> exact DTW (or zero fill) -> three numbers
// per pair.
//   set_mfcc            c[b][t][k-1] = sum_n x[b][t][n] cos(pi k (2n+1) / (2M)), k = 1..K: a plain fp32 FMA chain in ascending n against a
//                       host-built table; ~3 k MACs per frame.  The kernel is mfcc_kernel<false> of mfcc.h (wav_mcd.hip runs its other form).
//   set_dtw             the exact DTW of utils/metrics/dtw.py `accelerated_dtw(x, y, 'euclidean', warp=1)`.  One 256-thread block per pair;
//                       strips of 256 rows; thread t owns row i of the strip, holds x_i in registers and walks the columns skewed: at step
//                       s it is at column s - t, so the three predecessors of its cell were finished one and two steps earlier --
//                       D[i-1][j] is lane t-1's value of the step before (a lane shift; one double-buffered LDS slot per wave boundary),
//                       D[i-1][j-1] is what the same shift delivered a step earlier, D[i][j-1] is the thread's own last value.  The path
//                       length L travels with D.  y lives in LDS as a ring of 320 columns (the 256 a strip's diagonal spans plus the 64
//                       of the block being staged), row stride K padded to an odd count: the 64 lanes read 64 different columns without a
//                       bank conflict.  The strip's last row goes to a boundary buffer in LDS (Ty x (fp32 + int32)) and is the next
//                       strip's row above.  One barrier per step.  A block touches only its own pair: no inter-block dependencies, no
//                       spin-waits, no atomics.
//   set_dtw_path        one thread per pair walks `dir` back from the end and writes entry n from the back at index steps - 1 - n.
//   set_zero_fill_dist  sum_t ||x_t - y_t|| over t < max(len_x, len_y), the shorter side read as zeros; one block per pair, per-thread sums
//                       in ascending t, then a fixed LDS tree.
//   set_mcd_finish      mcd = num / frames, penalty = 2 - (len_1 + len_2) / frames.
// Costs are in the difference form sqrt(sum_k (x_ik - y_jk)^2): on integer grids every cost, every D and every comparison is exact.
#include "mfcc.h"  // mfcc_kernel<DB>, row_len, MCD_K_MAX / MCD_M_MAX: shared with wav_mcd.hip

namespace {

constexpr int DTW_ROWS = 256;                   // rows per strip = threads per block
constexpr int DTW_CB = 64;                      // columns staged at a time
constexpr int DTW_RING = DTW_ROWS + DTW_CB;     // columns the ring holds (a multiple of 64: the bank of a column survives the wrap)
constexpr int DTW_TY_MAX = 8192;                // boundary buffer: 8 bytes of LDS per column

constexpr int dtw_lds_bytes(int kp, int Ty) { return (DTW_RING * (kp + 1) + 2 * Ty + 16) * 4; }

template <int KP>
__global__ void __launch_bounds__(256) dtw_kernel(const float *__restrict__ x, const float *__restrict__ y, const int64_t *__restrict__ len_x,
                                                  const int64_t *__restrict__ len_y, float *__restrict__ dist, int32_t *__restrict__ steps,
                                                  uint8_t *__restrict__ dir, int Tx, int Ty, int K) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int YS = KP + 1;  // odd
    float *ring = lds;                                   // [DTW_RING][YS]: column j at slot j mod DTW_RING, entries k >= K zero
    float *bndD = ring + DTW_RING * YS;                  // [Ty] D of the row above the strip
    int *bndL = reinterpret_cast<int *>(bndD + Ty);      // [Ty] L of the same row
    float *xD = reinterpret_cast<float *>(bndL + Ty);    // [2][4] lane 63 of each wave, double-buffered by step parity
    int *xL = reinterpret_cast<int *>(xD + 8);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x;
    const int lx = row_len(len_x, b, 1, Tx), ly = row_len(len_y, b, 1, Ty);
    const float *__restrict__ xb = x + (int64_t)b * Tx * K;
    const float *__restrict__ yb = y + (int64_t)b * Ty * K;
    uint8_t *__restrict__ db = dir ? dir + (int64_t)b * Tx * Ty : nullptr;
    const float INF = __builtin_inff();

    for (int e = tid; e < DTW_RING * YS; e += 256) ring[e] = 0.0f;

    for (int i0 = 0; i0 < lx; i0 += DTW_ROWS) {
        const int i = i0 + tid;
        const bool live = i < lx;
        float xr[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) xr[k] = live && k < K ? xb[(int64_t)i * K + k] : 0.0f;
        const int nsteps = ly - 1 + min(DTW_ROWS, lx - i0);
        float cd = INF, pud = INF;  // this thread's last D; the D the shift delivered last step (next step's diagonal)
        int cl = 0, pul = 0;
        if (tid < 8) {
            xD[tid] = INF;
            xL[tid] = 0;
        }
        int slot = tid == 0 ? 0 : DTW_RING - tid;  // (s - tid) mod DTW_RING at s = 0
        __syncthreads();  // the ring zeroed / the strip before done with ring, slots and boundary row

        for (int s = 0; s < nsteps; ++s) {
            if ((s & (DTW_CB - 1)) == 0 && s < ly) {  // block-uniform: stage columns s .. s + 63 (nobody is left of column s - 255 any more)
                for (int e = tid; e < DTW_CB * K; e += 256) {
                    const int c = e / K, k = e - c * K, j = s + c;
                    ring[(j % DTW_RING) * YS + k] = j < ly ? yb[(int64_t)j * K + k] : 0.0f;
                }
                __syncthreads();
            }
            const int j = s - tid;
            float ud = __shfl_up(cd, 1);
            int ul = __shfl_up(cl, 1);
            if (lane == 0) {
                if (wv > 0) {  // written by lane 63 of the wave above at step s - 1
                    ud = xD[((s + 1) & 1) * 4 + wv - 1];
                    ul = xL[((s + 1) & 1) * 4 + wv - 1];
                } else if (i0 > 0 && s < ly) {
                    ud = bndD[s];
                    ul = bndL[s];
                } else {
                    ud = INF;
                    ul = 0;
                }
            }
            const float *yr = ring + slot * YS;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float d = xr[k] - yr[k];
                acc = __builtin_fmaf(d, d, acc);
            }
            const float c = __fsqrt_rn(acc);
            // ties go to the first of diagonal, i-1, j-1
            float best = pud;
            int bl = pul, dr = 0;
            if (ud < best) best = ud, bl = ul, dr = 1;
            if (cd < best) best = cd, bl = cl, dr = 2;
            if (i == 0 && j == 0) best = 0.0f, bl = 0, dr = 0;
            const bool act = live && j >= 0 && j < ly;
            cd = act ? c + best : INF;
            cl = act ? 1 + bl : 0;
            pud = ud;
            pul = ul;
            if (lane == 63 && wv < 3) {
                xD[(s & 1) * 4 + wv] = cd;
                xL[(s & 1) * 4 + wv] = cl;
            }
            if (act) {
                if (tid == DTW_ROWS - 1) {
                    bndD[j] = cd;
                    bndL[j] = cl;
                }
                if (db) db[(int64_t)i * Ty + j] = (uint8_t)dr;
                if (i == lx - 1 && j == ly - 1) {
                    dist[b] = cd;
                    steps[b] = cl;
                }
            }
            slot = slot + 1 == DTW_RING ? 0 : slot + 1;
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(64) dtw_path_kernel(const uint8_t *__restrict__ dir, const int64_t *__restrict__ len_x,
                                                      const int64_t *__restrict__ len_y, const int32_t *__restrict__ steps,
                                                      int32_t *__restrict__ path, int B, int Tx, int Ty) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int lx = row_len(len_x, b, 1, Tx), ly = row_len(len_y, b, 1, Ty);
    const int P = Tx + Ty - 1;
    const int n_path = min(max(steps[b], 0), P);
    const uint8_t *__restrict__ db = dir + (int64_t)b * Tx * Ty;
    int32_t *__restrict__ pb = path + (int64_t)b * P * 2;
    int i = lx - 1, j = ly - 1;
    for (int n = n_path - 1; n >= 0; --n) {  // entry n from the front; never outside [0, steps)
        pb[2 * n] = i;
        pb[2 * n + 1] = j;
        if (i == 0 && j == 0) break;
        const int d = db[(int64_t)i * Ty + j];
        // a move off the matrix is never taken, whatever the byte says
        if (j == 0 || (d == 1 && i > 0)) --i;
        else if (i == 0 || d == 2) --j;
        else --i, --j;
    }
}

__global__ void __launch_bounds__(256) zero_fill_dist_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                             const int64_t *__restrict__ len_x, const int64_t *__restrict__ len_y,
                                                             float *__restrict__ sum, int Tx, int Ty, int K) {
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int lx = row_len(len_x, b, 1, Tx), ly = row_len(len_y, b, 1, Ty);
    const int n = max(lx, ly);
    const float *__restrict__ xb = x + (int64_t)b * Tx * K;
    const float *__restrict__ yb = y + (int64_t)b * Ty * K;
    float part = 0.0f;
    for (int t = tid; t < n; t += 256) {
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float xv = t < lx ? xb[(int64_t)t * K + k] : 0.0f;
            const float yv = t < ly ? yb[(int64_t)t * K + k] : 0.0f;
            const float d = xv - yv;
            acc = __builtin_fmaf(d, d, acc);
        }
        part += __fsqrt_rn(acc);
    }
    red[tid] = part;
    for (int off = 128; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) red[tid] += red[tid + off];
    }
    if (tid == 0) sum[b] = red[0];
}

__global__ void __launch_bounds__(64) mcd_finish_kernel(const float *__restrict__ num, const int32_t *__restrict__ steps,
                                                        const int64_t *__restrict__ len_1, const int64_t *__restrict__ len_2,
                                                        float *__restrict__ mcd, float *__restrict__ penalty, int64_t *__restrict__ frames,
                                                        int B, int T1, int T2) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int l1 = row_len(len_1, b, 1, T1), l2 = row_len(len_2, b, 1, T2);
    const int fr = steps ? max(steps[b], 1) : max(l1, l2);
    mcd[b] = (float)((double)num[b] / (double)fr);
    penalty[b] = (float)(2.0 - (double)(l1 + l2) / (double)fr);
    frames[b] = fr;
}

}  // namespace

extern "C" int set_mfcc(const float *mel, const int64_t *lengths, const float *table, float *out, int32_t B, int32_t T, int32_t M, int32_t K,
                        int32_t take_log, void *stream) {
    SET_REQUIRE(mel && table && out, "set_mfcc");
    SET_REQUIRE(B > 0 && B <= 65535 && T > 0 && M > 0 && K > 0 && (take_log == 0 || take_log == 1), "set_mfcc");
    if (K > MCD_K_MAX || M > MCD_M_MAX) return set_fail(SET_E_UNSUPPORTED, "set_mfcc", "built for n_mfcc <= 64, n_mels <= 96");
    SET_REQUIRE((int64_t)B * T * M < (int64_t)1 << 40, "set_mfcc");
    const dim3 grid((T + MFCC_FR - 1) / MFCC_FR, B);
    hipLaunchKernelGGL(mfcc_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, mel, lengths, table, out, T, M, K, take_log,
                       (const float *)nullptr, 0.0f);
    return set_check_launch("set_mfcc");
}

extern "C" int set_dtw(const float *x, const float *y, const int64_t *len_x, const int64_t *len_y, float *dist, int32_t *steps, uint8_t *dir,
                       int32_t B, int32_t Tx, int32_t Ty, int32_t K, void *stream) {
    SET_REQUIRE(x && y && dist && steps, "set_dtw");
    SET_REQUIRE(B > 0 && Tx > 0 && Ty > 0 && K > 0, "set_dtw");
    if (K > MCD_K_MAX || Ty > DTW_TY_MAX) return set_fail(SET_E_UNSUPPORTED, "set_dtw", "built for K <= 64, Ty <= 8192");
    SET_REQUIRE((int64_t)Tx + Ty - 1 <= INT32_MAX && (int64_t)B * Tx * Ty < (int64_t)1 << 44, "set_dtw");
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, dtw_lds_bytes(64, DTW_TY_MAX), "set_dtw attr", dtw_kernel<40>, dtw_kernel<64>)) return rc;
    if (K <= 40)
        hipLaunchKernelGGL(dtw_kernel<40>, dim3(B), dim3(256), dtw_lds_bytes(40, Ty), (hipStream_t)stream, x, y, len_x, len_y, dist, steps, dir,
                           Tx, Ty, K);
    else
        hipLaunchKernelGGL(dtw_kernel<64>, dim3(B), dim3(256), dtw_lds_bytes(64, Ty), (hipStream_t)stream, x, y, len_x, len_y, dist, steps, dir,
                           Tx, Ty, K);
    return set_check_launch("set_dtw");
}

extern "C" int set_dtw_path(const uint8_t *dir, const int64_t *len_x, const int64_t *len_y, const int32_t *steps, int32_t *path, int32_t B,
                            int32_t Tx, int32_t Ty, void *stream) {
    SET_REQUIRE(dir && steps && path, "set_dtw_path");
    SET_REQUIRE(B > 0 && Tx > 0 && Ty > 0 && (int64_t)Tx + Ty - 1 <= INT32_MAX / 2, "set_dtw_path");
    hipLaunchKernelGGL(dtw_path_kernel, dim3(set_blocks(B, 64)), dim3(64), 0, (hipStream_t)stream, dir, len_x, len_y, steps, path, B, Tx, Ty);
    return set_check_launch("set_dtw_path");
}

extern "C" int set_zero_fill_dist(const float *x, const float *y, const int64_t *len_x, const int64_t *len_y, float *sum, int32_t B, int32_t Tx,
                                  int32_t Ty, int32_t K, void *stream) {
    SET_REQUIRE(x && y && sum, "set_zero_fill_dist");
    SET_REQUIRE(B > 0 && Tx > 0 && Ty > 0 && K > 0, "set_zero_fill_dist");
    if (K > MCD_K_MAX) return set_fail(SET_E_UNSUPPORTED, "set_zero_fill_dist", "built for K <= 64");
    hipLaunchKernelGGL(zero_fill_dist_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, y, len_x, len_y, sum, Tx, Ty, K);
    return set_check_launch("set_zero_fill_dist");
}

extern "C" int set_mcd_finish(const float *num, const int32_t *steps, const int64_t *len_1, const int64_t *len_2, float *mcd, float *penalty,
                              int64_t *frames, int32_t B, int32_t T1, int32_t T2, void *stream) {
    SET_REQUIRE(num && mcd && penalty && frames, "set_mcd_finish");
    SET_REQUIRE(B > 0 && T1 > 0 && T2 > 0, "set_mcd_finish");
    hipLaunchKernelGGL(mcd_finish_kernel, dim3(set_blocks(B, 64)), dim3(64), 0, (hipStream_t)stream, num, steps, len_1, len_2, mcd, penalty,
                       frames, B, T1, T2);
    return set_check_launch("set_mcd_finish");
}
