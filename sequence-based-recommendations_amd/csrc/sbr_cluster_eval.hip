// sbr_cluster_evaluate: whole test / validation users of a cluster model on the device (include/sbr_rnn.h; the chunk loop is in
// sbr_rank_api.hip next to sbr_evaluate).  Pack and hits are sbr_eval.hip's kernels, grouping, member scoring, gathering and
// translation sbr_cluster_rank.hip's, exclusion (of both rankings), select and sort sbr_rank.hip's.  What those do not do:
//   1. cev_transpose_kernel  hard [N][C] -> hardT [C][N], once per version of R
//   2. cev_product_kernel    softmax probability times hard membership of the row's cluster over the catalogue (PRODUCT road: the
//                            compiled test function, rnn_cluster.py:327-352), then +0.0 at the items fed
//   3. cev_use_kernel        users per selected cluster
// Rows are independent in every kernel; nothing waits on another workgroup.
#include "sbr_common.h"
#include "sbr_device.h"
#include <math.h>
#include <algorithm>

namespace {

// 32 x 32 tiles through LDS: reads and writes are both rows of 32 consecutive floats
__global__ void __launch_bounds__(256) cev_transpose_kernel(const float* __restrict__ in, int N, int C, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int n = n0 + j, c = c0 + tx;
        if (n < N && c < C) tile[j][tx] = in[(size_t)n * C + c];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, n = n0 + tx;
        if (n < N && c < C) out[(size_t)c * N + n] = tile[tx][j];
    }
}

// One workgroup per row: prod[r][i] = softmax(lg[r])[i] * hardT[csel[r]][i].  The probability is softmax_rows_kernel's float: the row
// already carries the bias (full_scores), the maximum is over the same values, and the sum, the reductions, expf and the multiply are
// the same calls (sbr_device.h) on the same lane-strided elements -- which is why a lane reads 4 bytes at stride 256 and not 16 bytes:
// another assignment of elements to lanes is another rounding of the sum.  A wave still reads 256 consecutive bytes per instruction.
// (Only the sum pass needs that assignment; the maximum and the write pass keep it for simplicity -- wider accesses there were not tried.)
// Then the items fed score +0.0 (numpy's s2[b, seen] = 0.0) and stay rankable.
__global__ void __launch_bounds__(256) cev_product_kernel(const float* __restrict__ lg, int N, int C, const int* __restrict__ csel,
                                                          const float* __restrict__ hardT, const int* __restrict__ items,
                                                          const long long* __restrict__ off, const int* __restrict__ users, int T,
                                                          int zero_fed, float* __restrict__ prod) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    const float* x = lg + (size_t)r * N;
    float* out = prod + (size_t)r * N;
    const int c = min(max(csel[r], 0), C - 1);       // (cl_select_kernel writes [0, C): the clamp only keeps the read in bounds)
    const float* m = hardT + (size_t)c * N;
    float mx = -INFINITY;
    for (int n = threadIdx.x; n < N; n += 256) mx = fmaxf(mx, x[n]);
    const float inv = softmax_row_scale(x, N, mx, red, mx);
    for (int n = threadIdx.x; n < N; n += 256) out[n] = softmax_row_value(x[n], mx, inv) * m[n];
    if (!zero_fed) return;
    __syncthreads();                                 // the row is written before a fed item is overwritten by another thread
    const int u = users[r];
    const long long o = off[u];
    const UserSplit sp(o, off[u + 1], T);
    for (int t = sp.window_begin() + threadIdx.x; t < sp.window_end(); t += 256) {
        const int id = items[o + t];
        if ((unsigned)id < (unsigned)N) out[id] = 0.0f;
    }
}

__global__ void __launch_bounds__(256) cev_use_kernel(const int* __restrict__ csel, long long n, int C, int* __restrict__ use) {
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        const int c = csel[j];
        if ((unsigned)c < (unsigned)C) atomicAdd(&use[c], 1);
    }
}

}  // namespace

hipError_t launch_cev_transpose(hipStream_t s, const float* hard, int N, int C, float* hardT) {
    cev_transpose_kernel<<<dim3((unsigned)((N + 31) / 32), (unsigned)((C + 31) / 32)), 256, 0, s>>>(hard, N, C, hardT);
    return hipGetLastError();
}

hipError_t launch_cev_product(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int T, int N, int C, int zero_fed,
                              const float* logits, const int* csel, const float* hardT, float* prod) {
    if (rows <= 0) return hipSuccess;
    cev_product_kernel<<<rows, 256, 0, s>>>(logits, N, C, csel, hardT, v.items, v.off, users, T, zero_fed, prod);
    return hipGetLastError();
}

hipError_t launch_cev_use(hipStream_t s, const int* csel, long long n, int C, int* use) {
    if (n <= 0) return hipSuccess;
    cev_use_kernel<<<(unsigned)std::min<long long>((n + 255) / 256, 1024), 256, 0, s>>>(csel, n, C, use);
    return hipGetLastError();
}
