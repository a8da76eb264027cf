// Device code that more than one translation unit must run the very same way: the block-wide reductions and the row softmax of the
// predict path (sbr_misc.hip: softmax_rows_kernel; sbr_cluster_eval.hip: cev_product_kernel -- its probability is the float
// sbr_predict_scores(probs = 1) writes, because both kernels call these functions), and the exclusion of every ranking call: where
// a row's excluded ids come from, where they land, and the binary search that removes one from a row of the compact cluster matrix.
#pragma once
#include "sbr_common.h"

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

// ---------------------------------------------------------------------------------------
// exclusion: "these ids of this row are not ranked", stated once for every ranking call (kernel and launcher: sbr_rank.hip)
// ---------------------------------------------------------------------------------------
// Where the excluded ids of row r come from.  Each of the four parts may be absent; the host fills the ones a call has.
struct ExclSources {
    const int* csr_ids = nullptr; const long long* csr_off = nullptr;      // the caller's lists: csr_ids[csr_off[r] .. csr_off[r + 1])
    const int* X = nullptr; const int* len = nullptr; int F = 1;           // the row's input window: X[r][t][0], t < min(len[r], T)
    const int* items = nullptr; const long long* off = nullptr;            // the dataset's CSR and the row's user: the viewed half
    const int* users = nullptr; int mode = SBR_EVAL_EXCL_NONE;             // (SBR_EVAL_EXCL_VIEWED) or the items fed (_WINDOW, _WINDOW_ZERO)
    int T = 0;
    // a session pool's slot of the row (sbr_sessions_rank): ring[slot][e % ring_len] holds the id of the slot's event e, events[slot] of
    // them were fed; SBR_SESSION_EXCL_LAST: the last one, _HISTORY: the last min(events, ses_history) -- never more than the ring keeps
    const int* ses_slots = nullptr; const int* ses_ring = nullptr; const long long* ses_events = nullptr;
    int ses_ring_len = 0, ses_history = 0, ses_mode = SBR_SESSION_EXCL_NONE;
    ExclSources& lists(const int* ids, const long long* offsets) { csr_ids = ids; csr_off = offsets; return *this; }
    ExclSources& window(const int* X_, const int* len_, int T_, int F_) { X = X_; len = len_; T = T_; F = F_; return *this; }
    ExclSources& dataset(const SbrEvalView& v, const int* users_, int T_, int mode_) {
        if (mode_ != SBR_EVAL_EXCL_NONE) { items = v.items; off = v.off; users = users_; mode = mode_; T = T_; }
        return *this;
    }
    ExclSources& sessions(const int* slots_, const int* ring_, const long long* events_, int ring_len_, int history_, int mode_) {
        if (mode_ != SBR_SESSION_EXCL_NONE) { ses_slots = slots_; ses_ring = ring_; ses_events = events_; ses_ring_len = ring_len_; ses_history = history_; ses_mode = mode_; }
        return *this;
    }
    bool any() const { return csr_off || X || users || ses_slots; }
};

// visit(id) for every excluded id of row r, the ids spread over the workgroup's threads; an id may come more than once and is not
// checked against any range here
template <class Visit>
__device__ __forceinline__ void excl_visit(const ExclSources& s, int r, Visit&& visit) {
    if (s.csr_off)
        for (long long j = s.csr_off[r] + threadIdx.x; j < s.csr_off[r + 1]; j += blockDim.x) visit(s.csr_ids[j]);
    if (s.X) {
        const int n = min(s.len[r], s.T);
        for (int t = threadIdx.x; t < n; t += blockDim.x) visit(s.X[((size_t)r * s.T + t) * s.F]);
    }
    if (s.users) {
        const int u = s.users[r];
        const UserSplit sp(s.off[u], s.off[u + 1], s.T);
        const int* seq = s.items + s.off[u];
        // VIEWED: every viewed item, also the ones in front of the window (top_k_recommendations, rnn_base.py:154-155); otherwise the
        // items fed (the compiled test function's exclude, rnn_base.py:200-202)
        for (int t = (s.mode == SBR_EVAL_EXCL_VIEWED ? sp.viewed_begin() : sp.window_begin()) + threadIdx.x; t < sp.viewed_end(); t += blockDim.x)
            visit(seq[t]);
    }
    if (s.ses_slots) {
        const int slot = s.ses_slots[r];
        const long long ev = s.ses_events[slot];
        const long long kept = s.ses_mode == SBR_SESSION_EXCL_LAST ? 1 : s.ses_history;
        const int n = (int)(ev < kept ? ev : kept);
        const int* ring = s.ses_ring + (size_t)slot * s.ses_ring_len;
        for (int t = threadIdx.x; t < n; t += blockDim.x) visit(ring[(ev - 1 - t) % s.ses_ring_len]);
    }
}

// Where they land.  A catalogue row: `value` at scores[r][id] -- -inf (never ranked: top_k_recommendations, rnn_base.py:154-155) or 0.0f
// (the compiled test function's scores * (1 - exclude) on raw outputs, :201-202, where the item stays rankable).
struct ExclCatalogue {
    float* scores; int N; float value;
    __device__ void exclude_row(const ExclSources& src, int r) const {
        float* row = scores + (size_t)r * N;
        excl_visit(src, r, [&](int id) { if ((unsigned)id < (unsigned)N) row[id] = value; });
    }
};
// A row of the compact cluster matrix cs [rows][lmax] (sbr_cluster_rank.hip): -inf at the id's place in the ascending member list of
// the row's cluster csel[r]; an id the cluster does not hold is ignored, and so is a row whose cluster is outside [0, C).
struct ExclCluster {
    float* cs; int lmax; const int* csel; int C; const int* mem; const int* moff; int N;
    __device__ void exclude_row(const ExclSources& src, int r) const {
        const int c = csel[r];
        if ((unsigned)c >= (unsigned)C) return;
        const int base = moff[c], n = min(moff[c + 1] - base, lmax);
        float* row = cs + (size_t)r * lmax;
        excl_visit(src, r, [&](int id) { if ((unsigned)id < (unsigned)N) crk_exclude_one(row, mem + base, n, id); });
    }
};
