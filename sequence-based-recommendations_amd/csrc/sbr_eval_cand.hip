// sbr_evaluate_candidates: every goal item of a user ranked among a candidate set of that user -- a list the caller brings, or
// negatives drawn on the device (include/sbr_rnn.h; host code: sbr_rank_api.hip).  Between sbr_evaluate_ranks' chunk
// loop (pack, forward) and the scoring sbr_rank_candidates already has (cand_score_kernel, or crk_gather_kernel from the full scores)
// the call needs two kernels, both reading the dataset's CSR (sbr_batch.hip) where it lies:
//   1. ev_cand_build_kernel   per row: [the draw of its negatives,] candidates and distinct goal items merged into one ascending list
//   2. ev_cand_place_kernel   per row: the mode's exclusion, then per goal place the count of rankable candidates in front of it
// What of a user's sequence is viewed, fed (the window) and the goal: UserSplit; the draw: ev_neg_seed / bb_draw_item (sbr_common.h).
// Rows are independent in both kernels; nothing waits on another workgroup.  Integer arithmetic only behind the scores.
#include "sbr_common.h"
#include <math.h>

namespace {

// first place of the ascending a[0 .. n) with a[place] >= x
__device__ __forceinline__ int lower_bound(const int* a, int n, int x) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// a thread's place among the threads of the workgroup that raise `f`, in thread order, and their number (ws: 4 words, free on return)
__device__ __forceinline__ int block_place(bool f, int* ws, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    int before = __popcll(b & ((1ull << lane) - 1));
    if (lane == 0) ws[w] = __popcll(b);
    __syncthreads();
    total = ws[0] + ws[1] + ws[2] + ws[3];
    for (int i = 0; i < w; ++i) before += ws[i];
    __syncthreads();
    return before;
}
static_assert(kEvCandThreads == 256, "block_place adds four waves");

__device__ __forceinline__ unsigned hash_slot(int item, unsigned mask) { return ((unsigned)item * 0x9E3779B1u >> 7) & mask; }

constexpr int kSeqSlots = 2 * kEvCandSeqLds;      // the hash set of a sequence of at most kEvCandSeqLds items: half full at the most

// One workgroup per row.
// Sampled (a.cand_ids == nullptr): the sequential rule of sbr_common.h, decided kEvCandThreads attempts at a time.  Thread i of a round
// draws attempt t = t0 + i and drops it when the item occurs in the user's sequence (L <= kEvCandSeqLds: a hash set of the sequence
// in LDS; longer: a binary search in the dataset's sorted goal half and a walk over the viewed half in memory).  The eligible items go
// into a hash set of LDS whose value is the LOWEST attempt that drew the item (integer atomic min: the result does not depend on the
// order of the threads): an attempt is the first of its item exactly when it finds its own t there, also against the rounds before.
// The first attempts in thread order take the next places of the accepted list; the draw ends at n_neg accepted or at the attempt cap.
// That is the list the sequential rule makes: an attempt is accepted iff it is eligible and no earlier attempt drew its item, and the
// accepted attempts are kept in attempt order up to n_neg.  The list is then sorted ascending in LDS (bitonic).
// Merge, both modes: E = the distinct goal ids inside the catalogue that are no candidates (the goal half comes sorted: a first
// occurrence differs from its left neighbour).  e of E lies at #{E < e} + #{candidates < e}, candidate i at i + #{e : lb(e) <= i}
// with lb(e) = #{candidates < e}; the goal is walked kEvCandThreads ids at a time, and the candidates in front of a round's last e
// are placed in that round.
__global__ void __launch_bounds__(kEvCandThreads) ev_cand_build_kernel(const int* __restrict__ items, const int* __restrict__ goal,
                                                                       const long long* __restrict__ off, EvCandBuild a, int P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_lb[kEvCandThreads];
    __shared__ int s_ws[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int u = a.users[r];
    const long long o = off[u];
    const UserSplit sp(o, off[u + 1], 0);                          // (no window here)
    const int L = sp.L, half = sp.half, ng = sp.goal_len();
    const int* seq = items + o;
    const int* gs = goal + o + half;                               // the goal half, sorted ascending
    const long long base = a.cap_off[r] - a.cap_off[0];
    const int cap = (int)(a.cap_off[r + 1] - a.cap_off[r]);
    int* out = a.mem + base;
    unsigned char* fl = a.flag + base;
    if (tid == 0) {
        a.moff[r] = (int)base; a.csel[r] = r;
        if (r == a.rows - 1) a.moff[a.rows] = (int)(a.cap_off[a.rows] - a.cap_off[0]);
    }

    const int* cand;
    int nc;
    if (a.cand_ids) {
        cand = a.cand_ids + a.cand_off[r];
        nc = a.cand_off[r + 1] - a.cand_off[r];
    } else {
        int* acc = (int*)smem;                                     // [P] the accepted items: draw order, then sorted
        int* hkey = acc + P;                                       // [hash_slots] the items drawn and eligible so far, -1: free
        int* hval = hkey + a.hash_slots;                           // [hash_slots] the lowest attempt that drew the item
        int* skey = hval + a.hash_slots;                           // [kSeqSlots] the user's sequence, when it fits
        const unsigned hmask = (unsigned)a.hash_slots - 1u;
        const bool seq_lds = L <= kEvCandSeqLds;
        for (int i = tid; i < a.hash_slots; i += kEvCandThreads) { hkey[i] = -1; hval[i] = 0x7fffffff; }
        if (seq_lds) for (int i = tid; i < kSeqSlots; i += kEvCandThreads) skey[i] = -1;
        __syncthreads();
        if (seq_lds)
            for (int i = tid; i < L; i += kEvCandThreads) {
                const int id = seq[i];
                if ((unsigned)id >= (unsigned)a.N) continue;       // never drawn
                unsigned h = hash_slot(id, kSeqSlots - 1);
                while (true) {
                    const int prev = atomicCAS(&skey[h], -1, id);
                    if (prev == -1 || prev == id) break;
                    h = (h + 1) & (kSeqSlots - 1);
                }
            }
        __syncthreads();
        const unsigned long long su = ev_neg_seed(a.seed, u);
        const int attempts = ev_neg_attempts(a.n_neg);
        int na = 0;
        for (int t0 = 0; t0 < attempts && na < a.n_neg; t0 += kEvCandThreads) {      // (uniform over the workgroup)
            const int t = t0 + tid;
            int item = -1, slot = 0;
            if (t < attempts) {
                const int it = bb_draw_item(su, t, a.cdf, a.N);
                bool seen = false;
                if (seq_lds) {
                    unsigned h = hash_slot(it, kSeqSlots - 1);
                    while (true) {
                        const int k = skey[h];
                        if (k == -1) break;
                        if (k == it) { seen = true; break; }
                        h = (h + 1) & (kSeqSlots - 1);
                    }
                } else {
                    const int p = lower_bound(gs, ng, it);
                    seen = p < ng && gs[p] == it;
                    for (int i = 0; i < half && !seen; ++i) seen = seq[i] == it;
                }
                if (!seen) item = it;
            }
            if (item >= 0) {
                unsigned h = hash_slot(item, hmask);
                while (true) {
                    const int prev = atomicCAS(&hkey[h], -1, item);
                    if (prev == -1 || prev == item) break;
                    h = (h + 1) & hmask;
                }
                atomicMin(&hval[h], t);
                slot = (int)h;
            }
            __syncthreads();
            const bool first = item >= 0 && hval[slot] == t;
            int total;
            const int place = na + block_place(first, s_ws, total);
            if (first && place < a.n_neg) acc[place] = item;
            na = min(a.n_neg, na + total);
        }
        __syncthreads();
        if (a.negatives)
            for (int i = tid; i < a.n_neg; i += kEvCandThreads) a.negatives[(size_t)r * a.n_neg + i] = i < na ? acc[i] : -1;
        __syncthreads();
        int P2 = 2;                                                // the sorted length: na rounded up to a power of two (P2 <= P)
        while (P2 < na) P2 <<= 1;
        for (int i = na + tid; i < P2; i += kEvCandThreads) acc[i] = 0x7fffffff;
        __syncthreads();
        for (int size = 2; size <= P2; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int q = tid; q < P2 / 2; q += kEvCandThreads) {
                    const int i = 2 * q - (q & (stride - 1)), j = i + stride;
                    const int x = acc[i], y = acc[j];
                    if ((x > y) == ((i & size) == 0)) { acc[i] = y; acc[j] = x; }
                }
                __syncthreads();
            }
        cand = acc;
        nc = na;
    }

    // --- the merge
    int n_e = 0, done = 0;                                         // goal-only entries and candidates placed so far
    for (int j0 = 0; j0 < ng; j0 += kEvCandThreads) {
        const int j = j0 + tid;
        int g = -1, lb = 0;
        bool emit = false;
        if (j < ng) {
            g = gs[j];
            if ((unsigned)g < (unsigned)a.N && (j == 0 || gs[j - 1] != g)) {
                lb = lower_bound(cand, nc, g);
                emit = !(lb < nc && cand[lb] == g);
            }
        }
        int total;
        const int e = block_place(emit, s_ws, total);
        if (emit) { s_lb[e] = lb; out[lb + n_e + e] = g; fl[lb + n_e + e] = 0; }
        __syncthreads();
        if (total) {
            const int upto = s_lb[total - 1];                      // the candidates in front of the round's last entry
            for (int i = done + tid; i < upto; i += kEvCandThreads) {
                int lo = 0, hi = total;                            // entries of the round with lb <= i
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_lb[mid] <= i) lo = mid + 1; else hi = mid; }
                out[i + n_e + lo] = cand[i]; fl[i + n_e + lo] = 1;
            }
            done = max(done, upto);
            n_e += total;
        }
        __syncthreads();                                           // s_lb is the next round's
    }
    for (int i = done + tid; i < nc; i += kEvCandThreads) { out[i + n_e] = cand[i]; fl[i + n_e] = 1; }
    const int len = nc + n_e;                                      // <= cap: the host's bound counts every goal place
    __syncthreads();
    const int pad = len ? out[len - 1] : 0;
    for (int i = len + tid; i < cap; i += kEvCandThreads) { out[i] = pad; fl[i] = 2; }
    if (tid == 0) a.mlen[r] = len;
}

// ---- the counts (ev_goal_rank_kernel's algorithm, sbr_eval.hip, over the compact row instead of the catalogue)
// An item's place is a count: the rankable candidates whose composite key << 32 | ~id is larger than its own (sbr_rank's order: key
// descending, ties to the lowest id).  One workgroup per row.  First the ids the mode excludes are searched in the row's ascending
// list and their scores set to -inf (the row is this call's scratch; equal values may be written twice).  Then the goal is taken
// kGoalRankTile places at a time: a place finds its item in the list (every goal item inside the catalogue is there), the tile's
// composites are sorted descending in LDS, every rankable CANDIDATE of the row (flag 1) finds by binary search how many of them are
// >= its own composite (p) and adds 1 to cnt[p], and after an inclusive scan the goal item whose composite first stands at place q of
// the sorted tile has scan[q] candidates in front of it.  A goal item that is itself a candidate has an equal composite there: not in
// front.  O((len + tile) log tile) per tile; a repeated goal item finds the same q at each of its places.
constexpr int kPlaceWaves = kRankThreads / 64;
constexpr int kPlaceCntWords = kGoalRankTile + 4;

__global__ void __launch_bounds__(kRankThreads) ev_cand_place_kernel(const int* __restrict__ items, const long long* __restrict__ off,
                                                                     const int* __restrict__ users, const long long* __restrict__ goal_off,
                                                                     int T, int N, int mode, const int* __restrict__ mem,
                                                                     const int* __restrict__ moff, const unsigned char* __restrict__ flag,
                                                                     const int* __restrict__ mlen, float* cs, int lmax,
                                                                     int* __restrict__ ranks, int* __restrict__ n_cand) {
    __shared__ unsigned long long c[kGoalRankTile];                // the tile's composites, sorted descending
    __shared__ unsigned cnt[kPlaceCntWords];                       // candidates per p, then its inclusive scan
    __shared__ unsigned ws[kPlaceWaves];
    __shared__ unsigned nrk;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int u = users[r];
    const long long o = off[u];
    const UserSplit sp(o, off[u + 1], T);
    const int ng = sp.goal_len();
    const int* seq = items + o;
    const int* g = seq + sp.half;                                  // the goal in sequence order
    const int* ids = mem + moff[r];
    const unsigned char* fl = flag + moff[r];
    const int len = mlen[r];                                       // <= lmax
    float* row = cs + (size_t)r * lmax;
    int* out = ranks + goal_off[r];
    if (tid == 0) nrk = 0;
    // VIEWED: every viewed item, also the ones in front of the window; WINDOW: the items fed (launch_exclude's dataset source)
    if (mode != SBR_EVAL_EXCL_NONE)
        for (int t = (mode == SBR_EVAL_EXCL_VIEWED ? sp.viewed_begin() : sp.window_begin()) + tid; t < sp.viewed_end(); t += kRankThreads) {
            const int id = seq[t];
            const int p = lower_bound(ids, len, id);
            if (p < len && ids[p] == id) row[p] = -INFINITY;
        }
    __syncthreads();

    for (int j0 = 0; j0 < ng; j0 += kGoalRankTile) {
        const int tn = min(kGoalRankTile, ng - j0);
        int P = 64;                                                // the sorted length: tn rounded up to a power of two, zero padded
        while (P < tn) P <<= 1;
        // --- 1. composites: thread t owns goal place j0 + t; an id outside the catalogue is not in the list and never ranked
        unsigned long long mine = 0ull;
        if (tid < tn) {
            const int gid = g[j0 + tid];
            const int p = lower_bound(ids, len, gid);
            const unsigned key = (p < len && ids[p] == gid) ? rank_key(row[p]) : 0u;
            mine = ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)gid);
        }
        if (tid < P) c[tid] = mine;
        cnt[tid] = 0;
        if (tid < kPlaceCntWords - kGoalRankTile) cnt[kGoalRankTile + tid] = 0;
        __syncthreads();
        // --- 2. bitonic sort, descending
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (tid < P / 2) {
                    const int i = 2 * tid - (tid & (stride - 1)), j = i + stride;
                    const unsigned long long x = c[i], y = c[j];
                    if ((x < y) == ((i & size) == 0)) { c[i] = y; c[j] = x; }
                }
                __syncthreads();
            }
        // --- 3. one pass over the row's candidates: p = #{ composites of the tile >= the candidate's own }; a candidate behind the
        // whole tile (p == tn) is in front of none of its goal items
        unsigned nr = 0;
        for (int i = tid; i < len; i += kRankThreads) {
            if (fl[i] != 1) continue;
            const unsigned key = rank_key(row[i]);
            if (key == 0u) continue;
            ++nr;
            const unsigned long long comp = ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)ids[i]);
            int lo = 0, hi = tn;                                   // first place with c[place] < comp
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid] >= comp) lo = mid + 1; else hi = mid; }
            if (lo < tn) atomicAdd(&cnt[lo], 1u);
        }
        if (j0 == 0) {
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1) nr += __shfl_xor(nr, o2);
            if (lane == 0) atomicAdd(&nrk, nr);
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
    if (tid == 0) n_cand[r] = (int)nrk;
}

}  // namespace

hipError_t launch_ev_cand_build(hipStream_t s, const SbrEvalView& v, const EvCandBuild& a) {
    if (a.rows <= 0) return hipSuccess;
    int P = 0;
    size_t lds = 0;
    if (!a.cand_ids) {
        if (a.n_neg < 1 || a.n_neg > SBR_EVAL_MAX_NEGATIVES || a.hash_slots != ev_neg_hash_slots(a.n_neg)) return hipErrorInvalidValue;
        P = 64;
        while (P < a.n_neg) P <<= 1;
        lds = ((size_t)P + 2 * (size_t)a.hash_slots + kSeqSlots) * sizeof(int);
        SBR_DYN_LDS(ev_cand_build_kernel, lds);
    }
    ev_cand_build_kernel<<<a.rows, kEvCandThreads, lds, s>>>(v.items, v.goal, v.off, a, P);
    return hipGetLastError();
}

hipError_t launch_ev_cand_place(hipStream_t s, const SbrEvalView& v, const int* users, const long long* goal_off, int rows, int T, int N,
                                int exclude_mode, const int* mem, const int* moff, const unsigned char* flag, const int* mlen, float* cs,
                                int lmax, int* ranks, int* n_cand) {
    if (rows <= 0) return hipSuccess;
    ev_cand_place_kernel<<<rows, kRankThreads, 0, s>>>(v.items, v.off, users, goal_off, T, N, exclude_mode, mem, moff, flag, mlen, cs, lmax,
                                                       ranks, n_cand);
    return hipGetLastError();
}
