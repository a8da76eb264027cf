// Device code that more than one translation unit must run the very same way: the block-wide reductions and the row softmax of the
// predict path (sbr_misc.hip: softmax_rows_kernel; sbr_cluster_eval.hip: cev_product_kernel -- its probability is the float
// sbr_predict_scores(probs = 1) writes, because both kernels call these functions), and the binary search that removes an id from a
// row of the compact cluster matrix (sbr_cluster_rank.hip, sbr_cluster_eval.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// ---------------------------------------------------------------------------------------
// block-wide reductions (256 threads = 4 waves)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.0f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = fmaxf(s, red[w]);
    return s;
}

// Softmax of one row x[0 .. N) of biased logits by a 256-thread workgroup.  mx_lane: the lane's maximum over its elements
// n = threadIdx.x, + 256, ...; on return mx is the row's maximum and the result 1 / sum exp(x - mx), the sum taken per lane over the same
// strided elements in ascending n, then over the lanes (wave_sum) and the four waves in order.  red: 4 floats of LDS.
__device__ __forceinline__ float softmax_row_scale(const float* x, int N, float mx_lane, float* red, float& mx) {
    mx = block_max(mx_lane, red);
    float se = 0.0f;
    for (int n = threadIdx.x; n < N; n += 256) se += expf(x[n] - mx);
    se = block_sum(se, red);
    return 1.0f / se;
}
__device__ __forceinline__ float softmax_row_value(float v, float mx, float inv) { return expf(v - mx) * inv; }

// -inf at the place of `id` in row[0 .. len), the scores of the ascending id list[0 .. len); nothing when the list does not hold it
__device__ __forceinline__ void crk_exclude_one(float* __restrict__ row, const int* __restrict__ list, int len, int id) {
    int lo = 0, hi = len;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (list[mid] < id) lo = mid + 1; else hi = mid; }
    if (lo < len && list[lo] == id) row[lo] = -INFINITY;
}
