// sbr_evaluate: whole test / validation users on the device (include/sbr_rnn.h; test.py:43-77, rnn_base.py:358-371 and the set
// algebra of evaluation.py:16-216).  Between the forward and the ranking kernels the call already has (sbr_rank.hip) it needs three
// small kernels, all reading the dataset's CSR (sbr_batch.hip) where it lies:
//   1. ev_pack_kernel      the rows fed: the last min(T, half) viewed items of every user of the chunk
//   2. ev_exclude_kernel   the viewed items out of the score rows
//   3. ev_hits_kernel      the ordered top-k against the goal: counts, the hit mask, per-item hit counts
// A user's sequence of L items is split at half = L / 2 (test.py:81-83): items[0 .. half) viewed, items[half .. L) the goal.
// Rows are independent in every kernel; nothing waits on another workgroup.
#include "sbr_common.h"
#include <math.h>

namespace {

// One wave per row of the batch buffers (what bb_pack_kernel writes for a training row, without targets and samples).
__global__ void __launch_bounds__(64) ev_pack_kernel(const int* __restrict__ items, const int* __restrict__ rate, const long long* __restrict__ off,
                                                     const int* __restrict__ users, int n_items, int rows, int T, int F, int* __restrict__ X,
                                                     int* __restrict__ lengths, float* __restrict__ pop) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= rows) {                                               // padded rows: index 0, length 0, popularity 1
        for (int t = lane; t < T * F; t += 64) X[(size_t)b * T * F + t] = 0;
        if (lane == 0) { lengths[b] = 0; pop[b] = 1.0f; }
        return;
    }
    const int u = users[b];
    const long long o = off[u];
    const int half = (int)(off[u + 1] - o) / 2;
    const int n_in = min(T, half), start = half - n_in;            // rnn_base.py:410: at most max_length items before the split
    for (int t = lane; t < T; t += 64) {
        X[((size_t)b * T + t) * F] = t < n_in ? items[o + start + t] : 0;
        if (F == 2) X[((size_t)b * T + t) * F + 1] = t < n_in ? n_items + rate[o + start + t] : 0;   // rnn_base.py:637-642
    }
    if (lane == 0) { lengths[b] = n_in; pop[b] = 1.0f; }
}

// One workgroup per row.  VIEWED: every viewed item, also the ones in front of the window (top_k_recommendations, rnn_base.py:154-155);
// WINDOW / WINDOW_ZERO: the items fed (the compiled test function's exclude, rnn_base.py:200-202) -- removed / scored 0.
__global__ void __launch_bounds__(256) ev_exclude_kernel(const int* __restrict__ items, const long long* __restrict__ off,
                                                         const int* __restrict__ users, int T, int N, int mode, float* __restrict__ scores) {
    const int r = blockIdx.x, u = users[r];
    const long long o = off[u];
    const int half = (int)(off[u + 1] - o) / 2;
    const int start = mode == SBR_EVAL_EXCL_VIEWED ? 0 : half - min(T, half);
    const float value = mode == SBR_EVAL_EXCL_WINDOW_ZERO ? 0.0f : -INFINITY;
    float* row = scores + (size_t)r * N;
    for (int t = start + threadIdx.x; t < half; t += blockDim.x) {
        const int id = items[o + t];
        if ((unsigned)id < (unsigned)N) row[id] = value;
    }
}

constexpr int kHitThreads = 256;

// One workgroup per row; a wave takes 64 consecutive places of the row's top-k at a time = two words of the hit mask.  A place is a hit
// when its id is found in the user's SORTED goal list (binary search: O(k log |goal|) per row whatever the lists hold); the ids of a row
// are distinct, so the hits counted per place are |set(goal) & set(top-k)| also when the goal repeats an item.  Integer counts only.
__global__ void __launch_bounds__(kHitThreads) ev_hits_kernel(const int* __restrict__ items, const int* __restrict__ goal,
                                                              const long long* __restrict__ off, const int* __restrict__ users, int k,
                                                              const int* __restrict__ ids, int* __restrict__ n_pred, int* __restrict__ hits,
                                                              int* __restrict__ first_hit, unsigned* __restrict__ mask, int* __restrict__ item_hits) {
    __shared__ int s_cnt[3];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int u = users[r];
    const long long o = off[u];
    const int L = (int)(off[u + 1] - o), half = L / 2, ng = L - half;
    const int* g = goal + o + half;
    const int first = items[o + half];                             // goal[0] of the sequence as it is, not of the sorted copy
    const int* irow = ids + (size_t)r * k;
    const int words = (k + 31) / 32;
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    int np = 0, nh = 0, nf = 0;
    for (int p0 = (tid >> 6) * 64; p0 < k; p0 += kHitThreads) {    // wave-uniform trip count
        const int p = p0 + lane;
        const int id = p < k ? irow[p] : -1;
        bool hit = false;
        if (id >= 0) {
            int lo = 0, hi = ng;                                   // first place with g[place] >= id
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (g[mid] < id) lo = mid + 1; else hi = mid; }
            hit = lo < ng && g[lo] == id;
        }
        const unsigned long long bh = __ballot(hit);
        np += __popcll(__ballot(id >= 0)); nh += __popcll(bh); nf += __popcll(__ballot(id >= 0 && id == first));
        if (hit && item_hits) atomicAdd(&item_hits[id], 1);
        if (mask && lane == 0) {
            const int w = p0 >> 5;
            mask[(size_t)r * words + w] = (unsigned)bh;
            if (w + 1 < words) mask[(size_t)r * words + w + 1] = (unsigned)(bh >> 32);
        }
    }
    if (lane == 0) { atomicAdd(&s_cnt[0], np); atomicAdd(&s_cnt[1], nh); atomicAdd(&s_cnt[2], nf); }
    __syncthreads();
    if (tid == 0) { n_pred[r] = s_cnt[0]; hits[r] = s_cnt[1]; first_hit[r] = s_cnt[2] > 0 ? 1 : 0; }
}

}  // namespace

hipError_t launch_ev_pack(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int Bp, int T, int F, int* X, int* lengths, float* pop) {
    if (Bp <= 0) return hipSuccess;
    ev_pack_kernel<<<Bp, 64, 0, s>>>(v.items, v.rate, v.off, users, v.n_items, rows, T, F, X, lengths, pop);
    return hipGetLastError();
}

hipError_t launch_ev_exclude(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int T, int N, int mode, float* scores) {
    if (rows <= 0 || mode == SBR_EVAL_EXCL_NONE) return hipSuccess;
    ev_exclude_kernel<<<rows, 256, 0, s>>>(v.items, v.off, users, T, N, mode, scores);
    return hipGetLastError();
}

hipError_t launch_ev_hits(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int k, const int* ids, int* n_pred, int* hits,
                          int* first_hit, unsigned* mask, int* item_hits) {
    if (rows <= 0) return hipSuccess;
    ev_hits_kernel<<<rows, kHitThreads, 0, s>>>(v.items, v.goal, v.off, users, k, ids, n_pred, hits, first_hit, mask, item_hits);
    return hipGetLastError();
}
