// Elementwise kernels with two access widths from one definition.  An op is a struct of pointers and sizes with
//     template <int W> __device__ void run(int64_t i) const;      // elements i .. i + W - 1
// and ew_launch() runs it with W = 4 (16-byte accesses, one index division per four elements: the one-element forms of these kernels
// ran at 2 - 4 TB/s) when the caller's `vec_ok` says that every unit is whole and 16-byte aligned, else with W = 1.  Both widths
// instantiate the same expressions and the library is built with -ffp-contract=off: the same bits per element.
// A loaded value is a float or an f32x4: + - * / act per element on either; ew_at / ew_set reach element e where an op needs a function
// call or a select per element (`for (e = 0; e < W; ++e)`).  tests/test_isa_schedule.py holds the W = 4 forms to dwordx4 accesses.
#pragma once
#include "common.h"

namespace {

template <int W> using ew_t = typename AVec<W>::type;  // float, f32x4
template <int W> __device__ __forceinline__ ew_t<W> ew_ld(const float *p) { return *reinterpret_cast<const ew_t<W> *>(p); }
template <int W> __device__ __forceinline__ void ew_st(float *p, ew_t<W> v) { *reinterpret_cast<ew_t<W> *>(p) = v; }
template <int W> __device__ __forceinline__ float ew_at(const ew_t<W> &v, int e) { return avec_get<W>(v, e); }
template <int W> __device__ __forceinline__ void ew_set(ew_t<W> &v, int e, float x) {
    if constexpr (W == 1) v = x; else v[e] = x;
}

template <int W, typename Op>
__global__ void __launch_bounds__(256) ew_kernel(Op op, int64_t units) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u < units) op.template run<W>(u * W);
}

template <typename Op>
inline int ew_launch(const Op &op, int64_t n, bool vec_ok, void *stream, const char *what) {
    if (vec_ok)
        hipLaunchKernelGGL((ew_kernel<4, Op>), dim3(set_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, op, n / 4);
    else
        hipLaunchKernelGGL((ew_kernel<1, Op>), dim3(set_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, op, n);
    return set_check_launch(what);
}

}  // namespace
