// The kernels of every ranking call (include/sbr_rnn.h: sbr_topk, sbr_rank, sbr_evaluate, sbr_cluster_rank, sbr_cluster_evaluate):
// ordered top-k of ANY depth with per-row exclusion (the batched form of top_k_recommendations, rnn_base.py:140-165).
//
// A row is read a bounded number of times, whatever k is:
//   1. exclude_kernel        the row's excluded ids -- whatever list, window or dataset names them -- leave a catalogue row or a
//                            compact cluster row (sources, sinks and the visiting loop: sbr_device.h)
//   2. rank_select_kernel    radix select of the k-th largest KEY (three digits: 11 + 11 + 10 bits, one LDS histogram each), then
//                            an ordered compaction: every candidate above that key, and the lowest ids among those equal to it
//                            until k is reached, leave the row IN ID ORDER -- which is the order equal keys must keep
//   3. rank_sort_*_kernel    the at most k entries by key descending (stable, or with the id in the composite: ties -> lowest id)
// One workgroup of kRankThreads threads per row in every kernel: rows are independent, nothing waits on another workgroup.
//
// KEY: the order-preserving 32-bit image of a score -- sign-flip transform of the float's bits, -0.0 canonicalised to +0.0 (the
// two compare equal as floats, so they must tie here), NaN and -inf (never ranked: an excluded or unusable item) mapped to
// 0, below every candidate (the smallest candidate, -FLT_MAX, has key 0x00800000).
#include "sbr_common.h"
#include "sbr_device.h"
#include <math.h>

namespace {

constexpr int kWaves = kRankThreads / 64;
constexpr int kBins = 2048;                       // bins of a select digit: two per thread for the suffix scan
constexpr int kSelFixedWords = kBins + 4 * kWaves;   // histogram, scan partials, per-wave counts (2), the found pair: 16-byte multiple
static_assert(kBins == 2 * kRankThreads, "the suffix scan of the select gives every thread two bins");
static_assert((kSelFixedWords * 4) % 16 == 0, "the LDS row starts on a 16-byte boundary");

// inclusive scan over the workgroup's kRankThreads values (ws: kWaves words of LDS, free again on return)
__device__ __forceinline__ unsigned block_incl_scan(unsigned v, unsigned* ws) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(v, o); if (lane >= o) v += t; }
    if (lane == 63) ws[w] = v;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < w; ++i) base += ws[i];
    __syncthreads();
    return v + base;
}

template <class Sink>
__global__ void __launch_bounds__(256) exclude_kernel(ExclSources src, Sink to) { to.exclude_row(src, blockIdx.x); }

// LDSROW: the row's keys are computed once into LDS and every pass reads them there (N <= kRankLdsRow); otherwise every pass
// streams the row from memory (one read per pass: 3 digits, the per-wave counts, the compaction).
template <bool LDSROW>
__global__ void __launch_bounds__(kRankThreads) rank_select_kernel(const float* __restrict__ scores, int N, int k, unsigned* __restrict__ keys,
                                                                   int* __restrict__ ids, int* __restrict__ n_sel) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* hist = (unsigned*)smem;             // [kBins]
    unsigned* ws = hist + kBins;                  // [kWaves]
    unsigned* wgt = ws + kWaves;                  // [kWaves] candidates above the threshold key in a wave's id segment
    unsigned* weq = wgt + kWaves;                 // [kWaves] ... equal to it
    unsigned* found = weq + kWaves;               // [2] the digit's result
    unsigned* lrow = (unsigned*)smem + kSelFixedWords;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = scores + (size_t)r * N;
    if (LDSROW) {
        for (int i = tid; i < N; i += kRankThreads) lrow[i] = rank_key(row[i]);
        __syncthreads();
    }
    auto key_at = [&](int i) -> unsigned { return LDSROW ? lrow[i] : rank_key(row[i]); };

    // --- the k-th largest key: one digit per pass, most significant first.  `remaining` = its place among the keys that share `prefix`
    unsigned prefix = 0, mask = 0, remaining = (unsigned)k;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        const unsigned dmask = pass == 2 ? 1023u : 2047u;
        for (int i = tid; i < kBins; i += kRankThreads) hist[i] = 0;
        __syncthreads();
        unsigned cur = 0, cnt = 0;                // scores crowd into a few bins: a thread adds a run of equal digits at once
        for (int i = tid; i < N; i += kRankThreads) {
            const unsigned key = key_at(i);
            if ((key & mask) == prefix) {
                const unsigned d = (key >> shift) & dmask;
                if (cnt && d == cur) ++cnt;
                else { if (cnt) atomicAdd(&hist[cur], cnt); cur = d; cnt = 1; }
            }
        }
        if (cnt) atomicAdd(&hist[cur], cnt);
        __syncthreads();
        // suffix sums from the top bin down: thread t owns bins kBins - 1 - 2t (hi) and kBins - 2 - 2t (lo)
        const unsigned c_hi = hist[kBins - 1 - 2 * tid], c_lo = hist[kBins - 2 - 2 * tid];
        const unsigned incl = block_incl_scan(c_hi + c_lo, ws), excl = incl - c_hi - c_lo;
        if (excl < remaining && remaining <= incl) {            // exactly one thread: 1 <= remaining <= keys sharing the prefix
            const bool hi = excl + c_hi >= remaining;
            found[0] = prefix | ((unsigned)(kBins - (hi ? 1 : 2) - 2 * tid) << shift);
            found[1] = remaining - excl - (hi ? 0u : c_hi);
        }
        __syncthreads();
        prefix = found[0]; remaining = found[1]; mask |= dmask << shift;
        __syncthreads();
    }
    // K = 0: the row has fewer than k candidates, all of them are above it and nothing equal to it is taken
    const unsigned K = prefix, need = remaining;

    // --- ordered compaction: wave w owns the ids [lo, hi); ranks inside a wave come from ballots, across waves from one table
    const int seg = ((N + kWaves - 1) / kWaves + 63) & ~63;
    const int lo = min(N, w * seg), hi = min(N, lo + seg);
    unsigned gt = 0, eq = 0;
    for (int i = lo + lane; i < hi; i += 64) { const unsigned key = key_at(i); gt += key > K; eq += key == K; }
    if (K == 0) eq = 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { gt += __shfl_xor(gt, o); eq += __shfl_xor(eq, o); }
    if (lane == 0) { wgt[w] = gt; weq[w] = eq; }
    __syncthreads();
    unsigned eq_run = 0, sel_run = 0;
    {
        unsigned e_all = 0, s_all = 0;
        for (int i = 0; i < kWaves; ++i) {
            if (i == w) { eq_run = e_all; sel_run = s_all; }
            const unsigned e = weq[i];
            s_all += wgt[i] + (e_all < need ? min(need - e_all, e) : 0u);
            e_all += e;
        }
        if (tid == 0) n_sel[r] = (int)min(s_all, (unsigned)k);
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned* krow = keys + (size_t)r * k;
    int* irow = ids + (size_t)r * k;
    for (int b = lo; b < hi; b += 64) {           // wave-uniform trip count
        const int i = b + lane;
        const bool valid = i < hi;
        const unsigned key = valid ? key_at(i) : 0u;
        const bool isgt = valid && key > K, iseq = valid && K != 0 && key == K;
        const unsigned long long beq = __ballot(iseq);
        const bool sel = isgt || (iseq && eq_run + (unsigned)__popcll(beq & lt) < need);
        const unsigned long long bsel = __ballot(sel);
        const unsigned pos = sel_run + (unsigned)__popcll(bsel & lt);
        if (sel && pos < (unsigned)k) { krow[pos] = key; irow[pos] = i; }
        eq_run += (unsigned)__popcll(beq); sel_run += (unsigned)__popcll(bsel);
    }
}

// the row's n entries and the places behind them, out of a sorted (key, id) list
__device__ __forceinline__ void rank_emit(const float* __restrict__ row, int N, int k, int n, int j, int id, int* __restrict__ oi,
                                          float* __restrict__ os) {
    const bool ok = j < n && (unsigned)id < (unsigned)N;
    oi[j] = ok ? id : -1;
    os[j] = ok ? row[id] : -INFINITY;
}

// k <= kRankSortLds: bitonic sort, descending, of the composites key << 32 | ~id in LDS (P = k rounded up to a power of two, zero padded:
// a real composite is never 0)
__global__ void __launch_bounds__(kRankThreads) rank_sort_lds_kernel(const float* __restrict__ scores, int N, int k, int P,
                                                                     const unsigned* __restrict__ keys, const int* __restrict__ ids,
                                                                     const int* __restrict__ n_sel, int* __restrict__ out_ids,
                                                                     float* __restrict__ out_scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* c = (unsigned long long*)smem;
    const int r = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = min(n_sel[r], k);
    const unsigned* krow = keys + (size_t)r * k;
    const int* irow = ids + (size_t)r * k;
    for (int i = tid; i < P; i += nt)
        c[i] = i < n ? ((unsigned long long)krow[i] << 32) | (unsigned long long)(0xffffffffu - (unsigned)irow[i]) : 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += nt) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long a = c[i], b = c[j];
                if ((a < b) == ((i & size) == 0)) { c[i] = b; c[j] = a; }
            }
            __syncthreads();
        }
    for (int j = tid; j < k; j += nt)
        rank_emit(scores + (size_t)r * N, N, k, n, j, j < n ? (int)(0xffffffffu - (unsigned)c[j]) : -1, out_ids + (size_t)r * k,
                  out_scores + (size_t)r * k);
}

// any k: stable LSD radix sort by key, descending, four 8-bit digits, between the row's two (key, id) buffers.  Wave w owns a
// contiguous piece of the list in every pass; tbl[digit][wave] -- digit-major, so one exclusive scan orders it -- is first the
// piece's digit counts, then the next free place of (digit, wave).  A wave moves its piece 64 entries at a time in list order:
// equal digits among the 64 find each other with eight ballots, and the last lane of a group advances the wave's place.
__global__ void __launch_bounds__(kRankThreads) rank_sort_radix_kernel(const float* __restrict__ scores, int N, int k, unsigned* keys0, int* ids0,
                                                                       unsigned* keys1, int* ids1, const int* __restrict__ n_sel,
                                                                       int* __restrict__ out_ids, float* __restrict__ out_scores) {
    __shared__ unsigned tbl[256 * kWaves];
    __shared__ unsigned ws[kWaves];
    static_assert(256 * kWaves == 4 * kRankThreads, "the scan of the table gives every thread four entries");
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = min(n_sel[r], k);
    unsigned *ka = keys0 + (size_t)r * k, *kb = keys1 + (size_t)r * k;
    int *ia = ids0 + (size_t)r * k, *ib = ids1 + (size_t)r * k;
    const int seg = ((n + kWaves - 1) / kWaves + 63) & ~63;
    const int lo = min(n, w * seg), hi = min(n, lo + seg);
    const unsigned long long lt = (1ull << lane) - 1ull;
    volatile unsigned* place = tbl;               // written by other lanes of the wave between two reads
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
        for (int i = tid; i < 256 * kWaves; i += kRankThreads) tbl[i] = 0;
        __syncthreads();
        for (int i = lo + lane; i < hi; i += 64) atomicAdd(&tbl[(255u - ((ka[i] >> shift) & 255u)) * kWaves + w], 1u);
        __syncthreads();
        {
            const unsigned a0 = tbl[4 * tid], a1 = tbl[4 * tid + 1], a2 = tbl[4 * tid + 2], a3 = tbl[4 * tid + 3];
            const unsigned s = a0 + a1 + a2 + a3, base = block_incl_scan(s, ws) - s;
            tbl[4 * tid] = base; tbl[4 * tid + 1] = base + a0; tbl[4 * tid + 2] = base + a0 + a1; tbl[4 * tid + 3] = base + a0 + a1 + a2;
        }
        __syncthreads();
        for (int b = lo; b < hi; b += 64) {       // wave-uniform trip count
            const int i = b + lane;
            const bool valid = i < hi;
            const unsigned key = valid ? ka[i] : 0u;
            const int id = valid ? ia[i] : 0;
            const unsigned dd = 255u - ((key >> shift) & 255u);
            unsigned long long m = __ballot(valid);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (dd >> bit) & 1u;
                const unsigned long long bb = __ballot(one);
                m &= one ? bb : ~bb;
            }
            const unsigned rank = (unsigned)__popcll(m & lt), cnt = (unsigned)__popcll(m);
            const unsigned pos = valid ? place[dd * kWaves + w] + rank : 0u;
            __builtin_amdgcn_wave_barrier();
            if (valid && pos < (unsigned)k) {
                kb[pos] = key; ib[pos] = id;
                if (rank + 1 == cnt) place[dd * kWaves + w] = pos + 1;
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        { unsigned* tk = ka; ka = kb; kb = tk; int* ti = ia; ia = ib; ib = ti; }
    }
    for (int j = tid; j < k; j += kRankThreads)   // four passes: the sorted list is back in the first buffer pair
        rank_emit(scores + (size_t)r * N, N, k, n, j, j < n ? ia[j] : -1, out_ids + (size_t)r * k, out_scores + (size_t)r * k);
}

}  // namespace

template <class Sink>
hipError_t launch_exclude(hipStream_t s, int rows, const ExclSources& src, const Sink& to) {
    if (rows <= 0 || !src.any()) return hipSuccess;
    exclude_kernel<<<rows, 256, 0, s>>>(src, to);
    return hipGetLastError();
}
template hipError_t launch_exclude<ExclCatalogue>(hipStream_t, int, const ExclSources&, const ExclCatalogue&);
template hipError_t launch_exclude<ExclCluster>(hipStream_t, int, const ExclSources&, const ExclCluster&);

hipError_t launch_rank_select(hipStream_t s, const float* scores, int rows, int N, int k, unsigned* keys, int* ids, int* n_sel, int* select) {
    *select = N <= kRankLdsRow ? 1 : 2;
    if (rows <= 0) return hipSuccess;
    const size_t fixed = (size_t)kSelFixedWords * sizeof(unsigned);
    if (N <= kRankLdsRow) {
        const size_t lds = fixed + ((size_t)N * sizeof(unsigned) + 15) / 16 * 16;
        SBR_DYN_LDS(rank_select_kernel<true>, lds);
        rank_select_kernel<true><<<rows, kRankThreads, lds, s>>>(scores, N, k, keys, ids, n_sel);
    } else
        rank_select_kernel<false><<<rows, kRankThreads, fixed, s>>>(scores, N, k, keys, ids, n_sel);
    return hipGetLastError();
}

hipError_t launch_rank_sort(hipStream_t s, const float* scores, int rows, int N, int k, unsigned* keys, int* ids, unsigned* keys2, int* ids2,
                            const int* n_sel, int* out_ids, float* out_scores, int* sort) {
    *sort = k <= kRankSortLds ? 1 : 2;
    if (rows <= 0) return hipSuccess;
    if (k <= kRankSortLds) {
        int P = 2;
        while (P < k) P <<= 1;
        const int threads = min(kRankThreads, max(64, P / 2));
        rank_sort_lds_kernel<<<rows, threads, (size_t)P * sizeof(unsigned long long), s>>>(scores, N, k, P, keys, ids, n_sel, out_ids, out_scores);
    } else
        rank_sort_radix_kernel<<<rows, kRankThreads, 0, s>>>(scores, N, k, keys, ids, keys2, ids2, n_sel, out_ids, out_scores);
    return hipGetLastError();
}
