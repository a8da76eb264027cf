// sbr_evaluate: whole test / validation users on the device (include/sbr_rnn.h; test.py:43-77, rnn_base.py:358-371 and the set
// algebra of evaluation.py:16-216).  Between the forward and the ranking kernels the call already has (sbr_rank.hip: exclusion --
// here of the viewed items, read from the dataset's CSR --, select, sort) it needs two small kernels, both reading the dataset's CSR
// (sbr_batch.hip) where it lies:
//   1. ev_pack_kernel      the rows fed: the window of every user of the chunk
//   2. ev_hits_kernel      the ordered top-k against the goal: counts, the hit mask, per-item hit counts
// and, for sbr_evaluate_ranks, in place of select + sort + 2:
//   3. ev_goal_rank_kernel the place of every goal item in the row's complete ranking, counted and never sorted out
// and, for sbr_evaluate_positions (the next item at every position of a sequence, from the states one forward pass leaves):
//   4. ev_pack_kernel<true>  the rows fed: the START of every user's sequence (UserPrefix)
//   5. ev_first_seen_kernel  per place of a row, whether its item occurs there for the first time
//   6. ev_next_rank_kernel   per position p, the place of x_p among the scores projected from slot p: one streamed count
// and, for sbr_evaluate_logprob / sbr_evaluate_positions_logprob (the log-probability of the same goal items):
//   7. row_log_z             the one float reduction of a score row, in an order fixed by N alone
//   8. ev_goal_logprob_kernel / ev_next_logprob_kernel / debug_row_logprob_kernel   its three launch shapes
// What of a user's sequence is viewed, fed (the window) and the goal: UserSplit (sbr_common.h).
// Rows are independent in every kernel; nothing waits on another workgroup.
#include "sbr_common.h"
#include <math.h>

namespace {

// One wave per row of the batch buffers (what bb_pack_kernel writes for a training row, without targets and samples).
// PREFIX: the split policy -- false: UserSplit's window (the end of the viewed half); true: UserPrefix's fed items (the start of the
// sequence, sbr_evaluate_positions).
template <bool PREFIX>
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
    const UserSplit sp(o, off[u + 1], T);
    const UserPrefix pf(o, off[u + 1], T, 1);
    // rnn_base.py:410: at most max_length items before the split; PREFIX: at most max_length items from the start, the last item never
    const int start = PREFIX ? 0 : sp.window_begin(), n_in = PREFIX ? pf.fed : sp.window_end() - start;
    for (int t = lane; t < T; t += 64) {
        X[((size_t)b * T + t) * F] = t < n_in ? items[o + start + t] : 0;
        if (F == 2) X[((size_t)b * T + t) * F + 1] = t < n_in ? n_items + rate[o + start + t] : 0;   // rnn_base.py:637-642
    }
    if (lane == 0) { lengths[b] = n_in; pop[b] = 1.0f; }
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
    const UserSplit sp(o, off[u + 1], 0);                          // (no window here)
    const int half = sp.half, ng = sp.goal_len();
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

// ---- sbr_evaluate_ranks: the place of every goal item in the complete ranking of its row
// An item's place is a count: the rankable items whose composite key << 32 | ~id is larger than its own (sbr_rank's order: key
// descending, ties to the lowest id).  One workgroup per row; the goal is taken kGoalRankTile items at a time, and per tile the row
// is read once: the tile's composites are sorted descending in LDS, every rankable item of the row finds by binary search how many of
// them are >= its own composite (p) and adds 1 to cnt[p] (integer LDS atomics: the sums do not depend on the order), and after an
// inclusive scan the goal item whose composite first stands at place q of the sorted tile has scan[q] items in front of it.
// O((N + tile) log tile) per tile whatever the goals hold; a repeated goal item finds the same q at each of its places.
constexpr int kGoalWaves = kRankThreads / 64;
constexpr int kGoalCntWords = kGoalRankTile + 4;                                   // cnt[p], p in [0, tile]; 16-byte multiple
constexpr int kGoalFixedBytes = kGoalRankTile * 8 + (kGoalCntWords + kGoalWaves + 4) * 4;   // composites, counts, scan partials, n_rankable
static_assert(kGoalFixedBytes % 16 == 0, "the LDS row starts on a 16-byte boundary");
static_assert(kGoalFixedBytes + kRankLdsRow * 4 <= 160 * 1024, "the row's keys and a tile's state share the CU's 160 KB");

// LDSROW: the row's keys are computed once into LDS (N <= kRankLdsRow); otherwise every tile streams the row from memory.
template <bool LDSROW>
__global__ void __launch_bounds__(kRankThreads) ev_goal_rank_kernel(const int* __restrict__ items, const long long* __restrict__ off,
                                                                    const int* __restrict__ users, const long long* __restrict__ goal_off,
                                                                    const float* __restrict__ scores, int N, int* __restrict__ ranks,
                                                                    int* __restrict__ n_rankable) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* c = (unsigned long long*)smem;             // [kGoalRankTile] the tile's composites, sorted descending
    unsigned* cnt = (unsigned*)(c + kGoalRankTile);                // [kGoalCntWords] items per p, then its inclusive scan
    unsigned* ws = cnt + kGoalCntWords;                            // [kGoalWaves]
    unsigned* nrk = ws + kGoalWaves;                               // [1] rankable items of the row
    unsigned* lrow = (unsigned*)(smem + kGoalFixedBytes);
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int u = users[r];
    const long long o = off[u];
    const UserSplit sp(o, off[u + 1], 0);                          // (no window here)
    const int ng = sp.goal_len();
    const int* g = items + o + sp.half;                            // the goal in sequence order
    int* out = ranks + goal_off[r];
    const float* row = scores + (size_t)r * N;
    if (tid == 0) nrk[0] = 0;
    if (LDSROW)
        for (int i = tid; i < N; i += kRankThreads) lrow[i] = rank_key(row[i]);
    __syncthreads();
    auto key_at = [&](int i) -> unsigned { return LDSROW ? lrow[i] : rank_key(row[i]); };

    for (int j0 = 0; j0 < ng; j0 += kGoalRankTile) {               // (ng >= 1: the call takes users of two items or more)
        const int tn = min(kGoalRankTile, ng - j0);
        int P = 64;                                                // the sorted length: tn rounded up to a power of two, zero padded
        while (P < tn) P <<= 1;
        // --- 1. composites: thread t owns goal item j0 + t; an id outside the catalogue is never ranked
        unsigned long long mine = 0ull;
        if (tid < tn) {
            const int gid = g[j0 + tid];
            const unsigned key = (unsigned)gid < (unsigned)N ? key_at(gid) : 0u;
            mine = ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)gid);
        }
        if (tid < P) c[tid] = mine;
        cnt[tid] = 0;
        if (tid < kGoalCntWords - kGoalRankTile) cnt[kGoalRankTile + tid] = 0;
        __syncthreads();
        // --- 2. bitonic sort, descending (rank_sort_lds_kernel's network)
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (tid < P / 2) {
                    const int i = 2 * tid - (tid & (stride - 1)), j = i + stride;
                    const unsigned long long a = c[i], b = c[j];
                    if ((a < b) == ((i & size) == 0)) { c[i] = b; c[j] = a; }
                }
                __syncthreads();
            }
        // --- 3. one pass over the row: p = #{ composites of the tile >= the item's own }; an item behind the whole tile (p == tn) is
        // in front of none of its goal items and is not counted.  A thread adds a run of equal p at once.
        unsigned cur = 0, run = 0, nr = 0;
        for (int i = tid; i < N; i += kRankThreads) {
            const unsigned key = key_at(i);
            if (key == 0u) continue;
            ++nr;
            const unsigned long long comp = ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
            int lo = 0, hi = tn;                                   // first place with c[place] < comp
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid] >= comp) lo = mid + 1; else hi = mid; }
            if (lo == tn) continue;
            if (run && (unsigned)lo == cur) ++run;
            else { if (run) atomicAdd(&cnt[cur], run); cur = (unsigned)lo; run = 1; }
        }
        if (run) atomicAdd(&cnt[cur], run);
        if (j0 == 0) {
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1) nr += __shfl_xor(nr, o2);
            if (lane == 0) atomicAdd(&nrk[0], nr);
        }
        __syncthreads();
        // --- 4. inclusive scan of cnt[0 .. kGoalRankTile): one word per thread
        unsigned v = cnt[tid];
#pragma unroll
        for (int o2 = 1; o2 < 64; o2 <<= 1) { const unsigned t = __shfl_up(v, o2); if (lane >= o2) v += t; }
        if (lane == 63) ws[w] = v;
        __syncthreads();
        for (int i = 0; i < w; ++i) v += ws[i];
        cnt[tid] = v;
        __syncthreads();
        // --- 5. the first place q of the item's own composite: everything counted at p <= q stands in front of it
        if (tid < tn) {
            int rank = -1;
            if ((unsigned)(mine >> 32) != 0u) {
                int lo = 0, hi = tn;                               // first place with c[place] <= mine
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid] > mine) lo = mid + 1; else hi = mid; }
                rank = (int)cnt[lo];
            }
            out[j0 + tid] = rank;
        }
        __syncthreads();                                           // c, cnt and ws are the next tile's
    }
    if (tid == 0) n_rankable[r] = (int)nrk[0];
}

// ---- sbr_evaluate_positions: the place of the NEXT item at every position of a row (UserPrefix, sbr_common.h)
// first[r][q] = 1 iff the item at place q of row r occurs at no place in front of q.  One workgroup per row, a thread per place,
// O(len^2) reads of a row of at most T ids, once per chunk: with the flags, taking the distinct items of the prefix x_0 .. x_{p-1} out
// of position p's counts is one pass over p places, not a search per place.
constexpr int kFirstSeenThreads = 256;
__global__ void __launch_bounds__(kFirstSeenThreads) ev_first_seen_kernel(const int* __restrict__ X, const int* __restrict__ lengths, int T, int F,
                                                                          int* __restrict__ first) {
    const int r = blockIdx.x;
    const int len = min(lengths[r], T);
    const int* x = X + (size_t)r * T * F;
    for (int q = threadIdx.x; q < len; q += kFirstSeenThreads) {
        const int id = x[(size_t)q * F];
        int seen = 0;
        for (int j = 0; j < q; ++j) seen |= (x[(size_t)j * F] == id);
        first[(size_t)r * T + q] = seen ? 0 : 1;
    }
}

// Position p of every row: one workgroup per (row, slot of the launch), rows with fewer than p items fed leave at once.  A slot's
// scores are the projection of slot p = p0 + blockIdx.y of the top layer's states -- what sbr_rank would rank for a row fed
// x_0 .. x_{p-1} -- and are only read.  The goal x_p comes from the
// dataset's CSR (the row holds the items FED: x_p is fed only when a later position exists).  One streamed pass over the N scores
// counts, in integers, the rankable items (key != 0) and those whose composite key << 32 | ~id is larger than the goal's (sbr_rank's
// order: key descending, ties to the lowest id); VEC: in 16-byte loads (N a multiple of 4: every row of scores then starts on a
// 16-byte boundary).  With exclude_prefix the flagged (= distinct) items of the prefix are taken back out of both counts, and the goal
// is never ranked when it is one of them.  Wave reduction by shuffles, then thread 0 adds the waves in order.
constexpr int kNextRankWaves = kRankThreads / 64;
struct NextCount { unsigned nr, ahead; };
__device__ __forceinline__ void next_count(float v, int i, unsigned long long gcomp, NextCount& c) {
    const unsigned key = rank_key(v);
    if (key == 0u) return;
    ++c.nr;
    const unsigned long long comp = ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
    c.ahead += comp > gcomp ? 1u : 0u;
}
template <bool VEC>
__global__ void __launch_bounds__(kRankThreads) ev_next_rank_kernel(const int* __restrict__ items, const long long* __restrict__ off,
                                                                    const int* __restrict__ users, const long long* __restrict__ pos_off,
                                                                    const int* __restrict__ X, const int* __restrict__ lengths,
                                                                    const int* __restrict__ first, int T, int F, int N, int p0, int min_history,
                                                                    int exclude_prefix, const float* __restrict__ scores, size_t slot_stride,
                                                                    int* __restrict__ ranks, int* __restrict__ n_rankable) {
    __shared__ unsigned s_w[kNextRankWaves][5];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = blockDim.x;
    const int p = p0 + blockIdx.y;                                 // slot blockIdx.y of the launch holds the scores of position p0 + blockIdx.y
    if (p > lengths[r]) return;                                    // (uniform over the workgroup) the row has no position p
    const int gid = items[off[users[r]] + p];                      // p <= fed <= L - 1: inside the user's sequence
    const float* row = scores + (size_t)blockIdx.y * slot_stride + (size_t)r * N;
    const bool gin = (unsigned)gid < (unsigned)N;                  // an id outside the catalogue is never ranked
    const unsigned gkey = gin ? rank_key(row[gid]) : 0u;
    const unsigned long long gcomp = ((unsigned long long)gkey << 32) | (unsigned long long)(0xffffffffu - (unsigned)gid);
    NextCount c{0u, 0u};
    if (VEC) {
        const float4* row4 = (const float4*)row;
        for (int i4 = tid; i4 < N / 4; i4 += nthreads) {
            const float4 v = row4[i4];
            next_count(v.x, 4 * i4, gcomp, c); next_count(v.y, 4 * i4 + 1, gcomp, c);
            next_count(v.z, 4 * i4 + 2, gcomp, c); next_count(v.w, 4 * i4 + 3, gcomp, c);
        }
    } else
        for (int i = tid; i < N; i += nthreads) next_count(row[i], i, gcomp, c);
    // the distinct items of the prefix: out of both counts; a thread per place of the row
    NextCount x{0u, 0u};
    unsigned gone = 0u;
    if (exclude_prefix) {
        const int* xr = X + (size_t)r * T * F;
        const int* fr = first + (size_t)r * T;
        for (int q = tid; q < p; q += nthreads) {                  // p <= lengths[r] <= T
            if (!fr[q]) continue;
            const int id = xr[(size_t)q * F];
            if ((unsigned)id >= (unsigned)N) continue;
            next_count(row[id], id, gcomp, x);
            gone |= (id == gid) ? 1u : 0u;
        }
    }
    unsigned v0 = c.nr, v1 = c.ahead, v2 = x.nr, v3 = x.ahead;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
        v0 += __shfl_xor(v0, o2); v1 += __shfl_xor(v1, o2); v2 += __shfl_xor(v2, o2); v3 += __shfl_xor(v3, o2);
        gone |= __shfl_xor(gone, o2);
    }
    if (lane == 0) { s_w[w][0] = v0; s_w[w][1] = v1; s_w[w][2] = v2; s_w[w][3] = v3; s_w[w][4] = gone; }
    __syncthreads();
    if (tid == 0) {
        unsigned nr = 0, ahead = 0, xnr = 0, xahead = 0, g = 0;
        for (int i = 0; i < nthreads / 64; ++i) {
            nr += s_w[i][0]; ahead += s_w[i][1]; xnr += s_w[i][2]; xahead += s_w[i][3]; g |= s_w[i][4];
        }
        const long long at = pos_off[r] + (p - min_history);
        ranks[at] = (gkey == 0u || g) ? -1 : (int)(ahead - xahead);
        n_rankable[at] = (int)(nr - xnr);
    }
}

// ---- sbr_sessions_replay_ranks: the place of every replayed event among the scores of the state in front of it
// One workgroup per row g0 + blockIdx.x of a pass's trace.  The pass row it belongs to is found by bisection over the rows' first
// trace rows (ascending); with that the event is items[pos], pos = start + (its place in the pass row), and it is event
// t = pos - first of the row's list in this call, the slot having had e0 + t events in front of it.  What sbr_sessions_rank would
// exclude then -- excl_visit's session window: the last min(e0 + t, kept) ids fed -- lies in the call's own events as far as they
// reach (x_{t-1} .. x_0) and beyond them in the ring as it stood BEFORE the call, kept aside by the host.  The pair's score row is
// its own (nobody else reads it), so the window's ids are written -inf there, as launch_exclude does for a ranking, behind one
// workgroup barrier; a repeated id is simply written twice, and a goal inside the window reads key 0 like any unrankable one.  Then
// ev_next_rank_kernel's streamed count (next_count, the same two load forms) and its reduction.
template <bool VEC>
__global__ void __launch_bounds__(kRankThreads) ses_event_rank_kernel(SesEventRank a) {
    __shared__ unsigned s_w[kNextRankWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthreads = blockDim.x;
    const long long g = a.g0 + blockIdx.x;
    int lo = 0, hi = a.n_rows - 1;                                 // the last pass row with at <= g (uniform)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.trows[mid].at <= g) lo = mid; else hi = mid - 1; }
    const SesTraceRow tw = a.trows[lo];
    const long long pos = a.rows[lo].start + (g - tw.at);
    const long long t = pos - tw.first, ev = a.keep_e0[tw.call_row] + t;
    const int gid = a.items[pos];
    float* row = a.scores + (size_t)blockIdx.x * a.N;
    const long long kept = a.mode == SBR_SESSION_EXCL_NONE ? 0 : a.mode == SBR_SESSION_EXCL_LAST ? 1 : a.history;
    const int nwin = (int)(ev < kept ? ev : kept);
    const int* ring = a.keep_ring + (size_t)tw.call_row * a.ring_len;
    for (int i = tid; i < nwin; i += nthreads) {
        const int id = i < t ? a.items[pos - 1 - i] : ring[(ev - 1 - i) % a.ring_len];
        if ((unsigned)id < (unsigned)a.N) row[id] = -INFINITY;
    }
    __syncthreads();
    const bool gin = (unsigned)gid < (unsigned)a.N;                // an id outside the catalogue is never ranked
    const unsigned gkey = gin ? rank_key(row[gid]) : 0u;
    const unsigned long long gcomp = ((unsigned long long)gkey << 32) | (unsigned long long)(0xffffffffu - (unsigned)gid);
    NextCount c{0u, 0u};
    if (VEC) {
        const float4* row4 = (const float4*)row;
        for (int i4 = tid; i4 < a.N / 4; i4 += nthreads) {
            const float4 v = row4[i4];
            next_count(v.x, 4 * i4, gcomp, c); next_count(v.y, 4 * i4 + 1, gcomp, c);
            next_count(v.z, 4 * i4 + 2, gcomp, c); next_count(v.w, 4 * i4 + 3, gcomp, c);
        }
    } else
        for (int i = tid; i < a.N; i += nthreads) next_count(row[i], i, gcomp, c);
    unsigned v0 = c.nr, v1 = c.ahead;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) { v0 += __shfl_xor(v0, o2); v1 += __shfl_xor(v1, o2); }
    if (lane == 0) { s_w[w][0] = v0; s_w[w][1] = v1; }
    __syncthreads();
    if (tid == 0) {
        unsigned nr = 0, ahead = 0;
        for (int i = 0; i < nthreads / 64; ++i) { nr += s_w[i][0]; ahead += s_w[i][1]; }
        a.ranks[pos] = gkey == 0u ? -1 : (int)ahead;
        a.n_rankable[pos] = (int)nr;
    }
}

// ---- sbr_evaluate_logprob, sbr_evaluate_positions_logprob, sbr_debug_row_logprob: the log-probability of the goal items under the
// softmax over the RANKABLE items of a score row.  Rankable: rank_key(v) != 0, the counting kernels' rule; m the largest
// rankable score, S the sum over the rankable items of exp(s_i - m); log_z = m + log(S), logp(g) = (s_g - m) - log(S).  A row without a
// rankable item has log_z = -inf; a goal that is not rankable (excluded, NaN, -inf, an id outside [0, N)) has logp = -inf.  A +inf
// score is rankable: m is then +inf, exp(s_i - m) is NaN at that item, and log_z and every logp of the row are NaN.  s_g - m below
// -3.4e38 (scores of both signs near the float range) rounds to -inf like any float subtraction.
// row_log_z is the one statement of the reduction, for all three launch shapes; the ORDER of its float additions is a function of N
// alone.  The row is taken in groups of four consecutive items, group q = items 4q .. 4q + 3 (the last one short when N is no
// multiple of 4); thread t of kLogpThreads -- a constant, never the launch's blockDim -- owns the groups t, t + kLogpThreads, .. and
// adds the terms of its groups in ascending item order into one float (at most 4 * ceil(ceil(N / 4) / kLogpThreads) terms); the
// kLogpThreads partials are then added by a fixed tree: six xor-shuffle levels inside each wave (offsets 32 .. 1), and the four wave
// sums as (w0 + w1) + (w2 + w3) -- depth 8.  No float atomics.  VEC only chooses how a group is LOADED (one 16-byte load, or up to
// four 4-byte loads): the same items meet the same thread in the same order.  Two passes over the row, the maximum and then the sum;
// the second finds the row in the cache.  Exclusion is never a subtraction from S: the excluded ids hold -inf in the row before the
// first pass (launch_exclude, or the prefix write of ev_next_logprob_kernel).
constexpr int kLogpThreads = 256;
constexpr int kLogpWaves = kLogpThreads / 64;
static_assert(kLogpWaves == 4, "row_log_z adds the wave sums as (w0 + w1) + (w2 + w3)");
struct RowLogZ { float m, log_s; };                                // log_z = m + log_s; no rankable item: m = log_s = -inf
template <bool VEC, class Term>
__device__ __forceinline__ void logp_groups(const float* row, int N, Term&& term) {
    const int groups = (N + 3) >> 2;
    for (int q = threadIdx.x; q < groups; q += kLogpThreads) {
        if (VEC) {                                                 // (N a multiple of 4: every group is whole)
            const float4 v = ((const float4*)row)[q];
            term(v.x); term(v.y); term(v.z); term(v.w);
        } else {
            const int i0 = 4 * q, n = min(4, N - i0);
            for (int j = 0; j < n; ++j) term(row[i0 + j]);
        }
    }
}
template <bool VEC>
__device__ __forceinline__ RowLogZ row_log_z(const float* row, int N, float* s_red /* [kLogpWaves] of LDS, free again on return */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float m = -INFINITY;
    logp_groups<VEC>(row, N, [&](float v) { if (rank_key(v) != 0u) m = fmaxf(m, v); });
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) m = fmaxf(m, __shfl_xor(m, o2));
    if (lane == 0) s_red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    __syncthreads();
    if (!(m > -INFINITY)) return RowLogZ{-INFINITY, -INFINITY};    // (uniform) no rankable item
    float sum = 0.0f;
    logp_groups<VEC>(row, N, [&](float v) { if (rank_key(v) != 0u) sum += expf(v - m); });
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) sum += __shfl_xor(sum, o2);   // a + b == b + a: both lanes of a pair hold the same bits
    if (lane == 0) s_red[w] = sum;
    __syncthreads();
    const float S = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    __syncthreads();
    return RowLogZ{m, logf(S)};
}
__device__ __forceinline__ float row_log_z_value(const RowLogZ& z) { return z.m > -INFINITY ? z.m + z.log_s : -INFINITY; }
// the goal's log-probability from the row as the reduction read it
__device__ __forceinline__ float goal_logp(const float* row, int N, int gid, const RowLogZ& z) {
    if ((unsigned)gid >= (unsigned)N) return -INFINITY;            // an id outside the catalogue is never ranked
    const float sg = row[gid];
    if (rank_key(sg) == 0u) return -INFINITY;
    return (sg - z.m) - z.log_s;
}

// One workgroup per row of a chunk, the goal items of sbr_evaluate_ranks: logp[goal_off[r] + j] for goal place j, log_z[r].  The row
// already holds -inf at what the call excludes.
template <bool VEC>
__global__ void __launch_bounds__(kLogpThreads) ev_goal_logprob_kernel(const int* __restrict__ items, const long long* __restrict__ off,
                                                                       const int* __restrict__ users, const long long* __restrict__ goal_off,
                                                                       const float* __restrict__ scores, int N, float* __restrict__ logp,
                                                                       float* __restrict__ log_z) {
    __shared__ float s_red[kLogpWaves];
    const int r = blockIdx.x;
    const int u = users[r];
    const long long o = off[u];
    const UserSplit sp(o, off[u + 1], 0);                          // (no window here)
    const float* row = scores + (size_t)r * N;
    const RowLogZ z = row_log_z<VEC>(row, N, s_red);
    const int* g = items + o + sp.half;                            // the goal in sequence order
    float* out = logp + goal_off[r];
    for (int j = threadIdx.x; j < sp.goal_len(); j += kLogpThreads) out[j] = goal_logp(row, N, g[j], z);
    if (threadIdx.x == 0 && log_z) log_z[r] = row_log_z_value(z);
}

// One workgroup per (row, position slot), the goal of ev_next_rank_kernel.  The (row, slot) score row belongs to this position alone:
// with exclude_prefix the ids of x_0 .. x_{p-1} are written -inf there behind one workgroup barrier (a repeated id is written twice),
// as ses_event_rank_kernel writes its window; the integer counts of the same position, where the call wants them, ran BEFORE this launch.
template <bool VEC>
__global__ void __launch_bounds__(kLogpThreads) ev_next_logprob_kernel(const int* __restrict__ items, const long long* __restrict__ off,
                                                                       const int* __restrict__ users, const long long* __restrict__ pos_off,
                                                                       const int* __restrict__ X, const int* __restrict__ lengths, int T, int F,
                                                                       int N, int p0, int min_history, int exclude_prefix, float* scores,
                                                                       size_t slot_stride, float* __restrict__ logp, float* __restrict__ log_z) {
    __shared__ float s_red[kLogpWaves];
    const int r = blockIdx.x;
    const int p = p0 + blockIdx.y;                                 // slot blockIdx.y of the launch holds the scores of position p0 + blockIdx.y
    if (p > lengths[r]) return;                                    // (uniform over the workgroup) the row has no position p
    const int gid = items[off[users[r]] + p];                      // p <= fed <= L - 1: inside the user's sequence
    float* row = scores + (size_t)blockIdx.y * slot_stride + (size_t)r * N;
    if (exclude_prefix) {
        const int* xr = X + (size_t)r * T * F;
        for (int q = threadIdx.x; q < p; q += kLogpThreads) {      // p <= lengths[r] <= T
            const int id = xr[(size_t)q * F];
            if ((unsigned)id < (unsigned)N) row[id] = -INFINITY;
        }
        __syncthreads();
    }
    const RowLogZ z = row_log_z<VEC>(row, N, s_red);
    if (threadIdx.x == 0) {
        const long long at = pos_off[r] + (p - min_history);
        logp[at] = goal_logp(row, N, gid, z);
        if (log_z) log_z[at] = row_log_z_value(z);
    }
}

// The test hook: the same device functions on the caller's rows, goals [rows][goals_per_row]
template <bool VEC>
__global__ void __launch_bounds__(kLogpThreads) debug_row_logprob_kernel(const float* __restrict__ scores, size_t ld, int N,
                                                                         const int* __restrict__ goal_ids, int goals_per_row,
                                                                         float* __restrict__ logp, float* __restrict__ log_z) {
    __shared__ float s_red[kLogpWaves];
    const int r = blockIdx.x;
    const float* row = scores + (size_t)r * ld;
    const RowLogZ z = row_log_z<VEC>(row, N, s_red);
    for (int j = threadIdx.x; j < goals_per_row; j += kLogpThreads)
        logp[(size_t)r * goals_per_row + j] = goal_logp(row, N, goal_ids[(size_t)r * goals_per_row + j], z);
    if (threadIdx.x == 0 && log_z) log_z[r] = row_log_z_value(z);
}

}  // namespace

// 16-byte loads: every row of the matrix starts on a 16-byte boundary and holds whole groups
static bool logp_vec(const float* scores, int N, size_t row_stride, size_t slot_stride = 0) {
    return N % 4 == 0 && row_stride % 4 == 0 && slot_stride % 4 == 0 && ((size_t)scores & 15) == 0;
}

hipError_t launch_ev_goal_logprob(hipStream_t s, const SbrEvalView& v, const int* users, const long long* goal_off, int rows, int N,
                                  const float* scores, float* logp, float* log_z, int* form) {
    const bool vec = logp_vec(scores, N, (size_t)N);
    *form = vec ? 1 : 2;
    if (rows <= 0) return hipSuccess;
    if (vec) ev_goal_logprob_kernel<true><<<rows, kLogpThreads, 0, s>>>(v.items, v.off, users, goal_off, scores, N, logp, log_z);
    else ev_goal_logprob_kernel<false><<<rows, kLogpThreads, 0, s>>>(v.items, v.off, users, goal_off, scores, N, logp, log_z);
    return hipGetLastError();
}

hipError_t launch_ev_next_logprob(hipStream_t s, const SbrEvalView& v, const int* users, const long long* pos_off, const int* X, const int* lengths,
                                  int rows, int T, int F, int N, int p0, int slots, int min_history, int exclude_prefix, float* scores,
                                  size_t slot_stride, float* logp, float* log_z, int* form) {
    const bool vec = logp_vec(scores, N, (size_t)N, slot_stride);
    *form = vec ? 1 : 2;
    if (rows <= 0 || slots <= 0) return hipSuccess;
    const dim3 grid(rows, slots);
    if (vec) ev_next_logprob_kernel<true><<<grid, kLogpThreads, 0, s>>>(v.items, v.off, users, pos_off, X, lengths, T, F, N, p0, min_history,
                                                                      exclude_prefix, scores, slot_stride, logp, log_z);
    else ev_next_logprob_kernel<false><<<grid, kLogpThreads, 0, s>>>(v.items, v.off, users, pos_off, X, lengths, T, F, N, p0, min_history,
                                                                     exclude_prefix, scores, slot_stride, logp, log_z);
    return hipGetLastError();
}

hipError_t launch_debug_row_logprob(hipStream_t s, const float* scores, size_t ld, int rows, int N, const int* goal_ids, int goals_per_row,
                                    float* logp, float* log_z, int* form) {
    const bool vec = logp_vec(scores, N, ld);
    *form = vec ? 1 : 2;
    if (rows <= 0) return hipSuccess;
    if (vec) debug_row_logprob_kernel<true><<<rows, kLogpThreads, 0, s>>>(scores, ld, N, goal_ids, goals_per_row, logp, log_z);
    else debug_row_logprob_kernel<false><<<rows, kLogpThreads, 0, s>>>(scores, ld, N, goal_ids, goals_per_row, logp, log_z);
    return hipGetLastError();
}

hipError_t launch_ses_event_rank(hipStream_t s, const SesEventRank& a, int rows, int* form) {
    const bool vec = a.N % 4 == 0;                                 // (the score rows start on 16-byte boundaries then: the scratch is carved in 256 bytes)
    *form = vec ? 1 : 2;
    if (rows <= 0) return hipSuccess;
    const int threads = a.N <= 16384 ? 256 : kRankThreads;         // as launch_ev_next_rank
    if (vec) ses_event_rank_kernel<true><<<rows, threads, 0, s>>>(a);
    else ses_event_rank_kernel<false><<<rows, threads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_ev_pack(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int Bp, int T, int F, int* X, int* lengths, float* pop) {
    if (Bp <= 0) return hipSuccess;
    ev_pack_kernel<false><<<Bp, 64, 0, s>>>(v.items, v.rate, v.off, users, v.n_items, rows, T, F, X, lengths, pop);
    return hipGetLastError();
}

hipError_t launch_ev_pack_prefix(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int Bp, int T, int F, int* X, int* lengths, float* pop) {
    if (Bp <= 0) return hipSuccess;
    ev_pack_kernel<true><<<Bp, 64, 0, s>>>(v.items, v.rate, v.off, users, v.n_items, rows, T, F, X, lengths, pop);
    return hipGetLastError();
}

hipError_t launch_ev_first_seen(hipStream_t s, const int* X, const int* lengths, int rows, int T, int F, int* first) {
    if (rows <= 0) return hipSuccess;
    ev_first_seen_kernel<<<rows, kFirstSeenThreads, 0, s>>>(X, lengths, T, F, first);
    return hipGetLastError();
}

hipError_t launch_ev_next_rank(hipStream_t s, const SbrEvalView& v, const int* users, const long long* pos_off, const int* X, const int* lengths,
                               const int* first, int rows, int T, int F, int N, int p0, int slots, int min_history, int exclude_prefix,
                               const float* scores, size_t slot_stride, int* ranks, int* n_rankable, int* form) {
    const bool vec = N % 4 == 0 && slot_stride % 4 == 0;
    *form = vec ? 1 : 2;
    if (rows <= 0 || slots <= 0) return hipSuccess;
    // a thread takes a few 16-byte loads at least: 256 threads up to 16 384 items, the select kernels' 1024 above
    const int threads = N <= 16384 ? 256 : kRankThreads;
    const dim3 grid(rows, slots);
    if (vec) ev_next_rank_kernel<true><<<grid, threads, 0, s>>>(v.items, v.off, users, pos_off, X, lengths, first, T, F, N, p0, min_history,
                                                                exclude_prefix, scores, slot_stride, ranks, n_rankable);
    else ev_next_rank_kernel<false><<<grid, threads, 0, s>>>(v.items, v.off, users, pos_off, X, lengths, first, T, F, N, p0, min_history,
                                                             exclude_prefix, scores, slot_stride, ranks, n_rankable);
    return hipGetLastError();
}

hipError_t launch_ev_hits(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int k, const int* ids, int* n_pred, int* hits,
                          int* first_hit, unsigned* mask, int* item_hits) {
    if (rows <= 0) return hipSuccess;
    ev_hits_kernel<<<rows, kHitThreads, 0, s>>>(v.items, v.goal, v.off, users, k, ids, n_pred, hits, first_hit, mask, item_hits);
    return hipGetLastError();
}

hipError_t launch_ev_goal_rank(hipStream_t s, const SbrEvalView& v, const int* users, const long long* goal_off, int rows, int N,
                               const float* scores, int* ranks, int* n_rankable, int* form) {
    *form = N <= kRankLdsRow ? 1 : 2;
    if (rows <= 0) return hipSuccess;
    if (N <= kRankLdsRow) {
        const size_t lds = (size_t)kGoalFixedBytes + ((size_t)N * sizeof(unsigned) + 15) / 16 * 16;
        SBR_DYN_LDS(ev_goal_rank_kernel<true>, lds);
        ev_goal_rank_kernel<true><<<rows, kRankThreads, lds, s>>>(v.items, v.off, users, goal_off, scores, N, ranks, n_rankable);
    } else
        ev_goal_rank_kernel<false><<<rows, kRankThreads, kGoalFixedBytes, s>>>(v.items, v.off, users, goal_off, scores, N, ranks, n_rankable);
    return hipGetLastError();
}
