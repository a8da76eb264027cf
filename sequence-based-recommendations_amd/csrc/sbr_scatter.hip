// K6, the scatter-add of the index-input gradient (gfx950, wave64): the counting sort of the batch's ids, the six forms of the
// scatter-add (sbr_query "scatter_form"), and sbr_scat_plan at the end: which form a shape takes, decided once in sbr_create.
#include "sbr_common.h"
#include "sbr_rec_p.h"      // f32x4 (sbr_cell.h), the pollers' helpers, tail_monitor_loop

// ---------------------------------------------------------------------------------------
// K6 scatter-add: dWin[X[b][t][f]][:] += dxt[t][b][:] for t < len[b]; duplicates accumulate
// (gradient of the advanced-indexing gather [3P]).
//
// Item ids follow a Zipf law, so per-element float atomics serialise in L2 on the popular rows
// (772 us at B=256, T=200, N=3706).  Instead the (position, id) pairs are counting-sorted by id
// (3 tiny integer kernels that depend only on the batch, run on a side stream under the BPTT
// chain), and one wave per chunk of 32 sorted entries sums the dxt rows of equal id in registers:
// rows are read once, coalesced, 16 B/lane; a row of dWin that lies entirely inside one chunk is
// written with plain stores, only segments that straddle a chunk boundary use atomics.
// ---------------------------------------------------------------------------------------
// Zipf ids: thousands of entries share the hottest id, so per-entry global atomics on cnt[]/cur[]
// serialise in one L2 channel (69 us each, and they slow every kernel running beside them).  For
// catalogues whose counters fit LDS (n_ids <= SCAT_LDS_IDS) each workgroup histograms its slice in
// LDS and issues ONE global atomic per distinct id it saw.
#define SCAT_LDS_IDS 36864    // 144 KB of LDS counters: catalogues up to ~37 k ids (C4's 26 744) take the LDS path
#define SCAT_BLOCK 1024
// Time-chunked keys (tch > 0): key = (t / tch) * ids_per_chunk + id, so that the entries of one chunk of time steps are
// contiguous in the sorted order and sorted by id inside it -- the scatter-add of a chunk can then run as soon as the BPTT
// chain has left that chunk (sbr_backward_recurrent, "tail overlap").  n_ids is the size of the KEY space.
__device__ __forceinline__ int scat_key(int id, int t, const SbrTChunks& tc, int ids_per_chunk) {
    if (tc.n <= 1) return id;
    int c = 0;
#pragma unroll
    for (int k = 1; k < SBR_TCHUNKS_MAX; ++k) c += (k < tc.n && t >= tc.lo[k]) ? 1 : 0;
    return c * ids_per_chunk + id;
}

__global__ void __launch_bounds__(SCAT_BLOCK) scat_count_lds_kernel(const int* __restrict__ X, const int* __restrict__ len,
                                                                    int T, int Bp, int F, int n_ids, int per_block,
                                                                    int* __restrict__ cnt, SbrTChunks tch, int ipc) {
    extern __shared__ int hist[];
    for (int i = threadIdx.x; i < n_ids; i += SCAT_BLOCK) hist[i] = 0;
    __syncthreads();
    const int total = T * Bp * F;
    const int lo = blockIdx.x * per_block, hi = min(total, lo + per_block);
    for (int i = lo + threadIdx.x; i < hi; i += SCAT_BLOCK) {
        const int f = i % F, pos = i / F, b = pos % Bp, t = pos / Bp;
        if (t < len[b]) atomicAdd(&hist[scat_key(X[((size_t)b * T + t) * F + f], t, tch, ipc)], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_ids; i += SCAT_BLOCK) { const int c = hist[i]; if (c) atomicAdd(&cnt[i], c); }
}

__global__ void __launch_bounds__(SCAT_BLOCK) scat_fill_lds_kernel(const int* __restrict__ X, const int* __restrict__ len,
                                                                   int T, int Bp, int F, int n_ids, int per_block,
                                                                   int* __restrict__ cur, int* __restrict__ sid,
                                                                   int* __restrict__ spos, int concat, SbrTChunks tch, int ipc) {
    extern __shared__ int hist[];          // [n_ids] counts, then cursors
    for (int i = threadIdx.x; i < n_ids; i += SCAT_BLOCK) hist[i] = 0;
    __syncthreads();
    const int total = T * Bp * F;
    const int lo = blockIdx.x * per_block, hi = min(total, lo + per_block);
    for (int i = lo + threadIdx.x; i < hi; i += SCAT_BLOCK) {
        const int f = i % F, pos = i / F, b = pos % Bp, t = pos / Bp;
        if (t < len[b]) atomicAdd(&hist[scat_key(X[((size_t)b * T + t) * F + f], t, tch, ipc)], 1);
    }
    __syncthreads();
    // reserve a contiguous slot range per id with one global atomic; hist[id] becomes the block's cursor
    for (int i = threadIdx.x; i < n_ids; i += SCAT_BLOCK) { const int c = hist[i]; if (c) hist[i] = atomicAdd(&cur[i], c); }
    __syncthreads();
    for (int i = lo + threadIdx.x; i < hi; i += SCAT_BLOCK) {
        const int f = i % F, pos = i / F, b = pos % Bp, t = pos / Bp;
        if (t < len[b]) {
            const int id = scat_key(X[((size_t)b * T + t) * F + f], t, tch, ipc);
            const int slot = atomicAdd(&hist[id], 1);
            sid[slot] = id; spos[slot] = concat ? i : pos;
        }
    }
}

// exclusive scan of cnt[0..n) -> offs[0..n], offs[n] = total; cur = copy of offs (fill cursors); one workgroup.
// LDS (n <= SCAT_LDS_IDS, e.g. the ~30 k keys of the time-chunked sort): the counters are staged in LDS with coalesced loads,
// every thread sums a contiguous run of ceil(n / 1024) of them, the 1024 run sums are scanned across the block once, every
// thread turns its run into prefixes in place, and the result leaves with coalesced stores.  Otherwise (large catalogues):
// one block-wide scan per 1024 counters, coalesced accesses throughout.
template <bool LDS>
__global__ void __launch_bounds__(1024) scat_scan_kernel(int* __restrict__ cnt, int n, int* __restrict__ offs,
                                                         int* __restrict__ cur) {
    extern __shared__ int stage[];
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!LDS) {
        if (threadIdx.x == 0) carry_s = 0;
        __syncthreads();
        for (int base = 0; base < n; base += 1024) {
            const int i = base + threadIdx.x;
            const int v = i < n ? cnt[i] : 0;
            int incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            int woff = 0;
            for (int w = 0; w < wave; ++w) woff += wsum[w];
            const int carry = carry_s;
            const int excl = carry + woff + incl - v;
            if (i < n) { offs[i] = excl; cur[i] = excl; }
            __syncthreads();
            if (threadIdx.x == 1023) carry_s = carry + woff + incl;
            __syncthreads();
        }
        if (threadIdx.x == 0) offs[n] = carry_s;
        return;
    }
    for (int i = threadIdx.x; i < n; i += 1024) { stage[i] = cnt[i]; cnt[i] = 0; }     // (zero again: the next sort of this shape needs no memset)
    __syncthreads();
    const int per = (n + 1023) / 1024;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += stage[i];
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    int run = woff + incl - sum;                      // exclusive prefix of this thread's run
    for (int i = lo; i < hi; ++i) { const int c = stage[i]; stage[i] = run; run += c; }
    if (threadIdx.x == 1023) offs[n] = woff + incl;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) { const int v = stage[i]; offs[i] = v; cur[i] = v; }
}

// Large catalogues (the counters do not fit LDS): three small launches instead of one workgroup walking the whole array
// (1 M counters took it 2 ms: a thousand rounds of three barriers) -- per 4096-counter block the local exclusive prefixes
// and the block's total; the totals' exclusive scan (one workgroup; parked in `cnt`, which nobody reads any more); the add.
constexpr int SCAN_BLK = 4096;
__global__ void __launch_bounds__(1024) scat_scan_local_kernel(const int* __restrict__ cnt, int n, int* __restrict__ offs,
                                                               int* __restrict__ bsum) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * SCAN_BLK + threadIdx.x * 4;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? cnt[i0 + k] : 0;
    const int mine = v[0] + v[1] + v[2] + v[3];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    int run = woff + incl - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (i0 + k < n) offs[i0 + k] = run; run += v[k]; }
    if (threadIdx.x == 1023) bsum[blockIdx.x] = run;
}
__global__ void __launch_bounds__(1024) scat_scan_totals_kernel(const int* __restrict__ bsum, int nb, int* __restrict__ bpre,
                                                                int* __restrict__ total) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int carry = carry_s;
        if (i < nb) bpre[i] = carry + woff + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}
__global__ void __launch_bounds__(1024) scat_scan_add_kernel(const int* __restrict__ bpre, int n, int* __restrict__ offs,
                                                             int* __restrict__ cur) {
    const int carry = bpre[blockIdx.x];
    const int i0 = blockIdx.x * SCAN_BLK + threadIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < n) { const int v = offs[i0 + k] + carry; offs[i0 + k] = v; cur[i0 + k] = v; }
}

// The counting sort of catalogues beyond the LDS histogram, round 6: one global atomic per DISTINCT id of a workgroup's 1 024 entries
// instead of one per entry.  The kernels this replaced sent every entry's atomic to cnt[id] / cur[id]; atomics on one address serialise
// at its L2 channel, and a step's hottest id holds thousands of its 51 200 entries (C5's batch: 3 612) -- ~50 us per kernel, all of it the
// hot counters, beside the head whose loads wait behind them (profiles/round6_variants.txt, calls s3 / a2).  Here a workgroup first
// groups its entries in an LDS hash table (id -> count; LDS atomics), then adds each distinct id's count once; the fill takes a base slot
// per distinct id the same way and every entry adds its rank inside the workgroup.
#define SCAT_AGG_SLOTS 2048
__device__ __forceinline__ int scat_agg_insert(int* __restrict__ hkey, int* __restrict__ hcnt, int id, int& rank) {
    unsigned h = ((unsigned)id * 2654435761u) >> 21;                  // 11 bits
    for (;;) {
        const int prev = atomicCAS(&hkey[h], -1, id);
        if (prev == -1 || prev == id) { rank = atomicAdd(&hcnt[h], 1); return (int)h; }
        h = (h + 1) & (SCAT_AGG_SLOTS - 1);
    }
}
__global__ void __launch_bounds__(1024) scat_count_agg_kernel(const int* __restrict__ X, const int* __restrict__ len, int T, int Bp, int F,
                                                              int* __restrict__ cnt) {
    __shared__ int hkey[SCAT_AGG_SLOTS], hcnt[SCAT_AGG_SLOTS];
    for (int k = threadIdx.x; k < SCAT_AGG_SLOTS; k += 1024) { hkey[k] = -1; hcnt[k] = 0; }
    __syncthreads();
    const int total = T * Bp * F, i = blockIdx.x * 1024 + threadIdx.x;
    if (i < total) {
        const int f = i % F, pos = i / F, b = pos % Bp, t = pos / Bp;
        if (t < len[b]) { int rank; (void)scat_agg_insert(hkey, hcnt, X[((size_t)b * T + t) * F + f], rank); }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SCAT_AGG_SLOTS; k += 1024) if (hkey[k] >= 0) atomicAdd(&cnt[hkey[k]], hcnt[k]);
}
__global__ void __launch_bounds__(1024) scat_fill_agg_kernel(const int* __restrict__ X, const int* __restrict__ len, int T, int Bp, int F,
                                                             int* __restrict__ cur, int* __restrict__ sid, int* __restrict__ spos, int concat) {
    __shared__ int hkey[SCAT_AGG_SLOTS], hcnt[SCAT_AGG_SLOTS], hbase[SCAT_AGG_SLOTS];
    for (int k = threadIdx.x; k < SCAT_AGG_SLOTS; k += 1024) { hkey[k] = -1; hcnt[k] = 0; }
    __syncthreads();
    const int total = T * Bp * F, i = blockIdx.x * 1024 + threadIdx.x;
    int id = -1, pos = 0, rank = 0, h = 0;
    if (i < total) {
        const int f = i % F; pos = i / F;
        const int b = pos % Bp, t = pos / Bp;
        if (t < len[b]) { id = X[((size_t)b * T + t) * F + f]; h = scat_agg_insert(hkey, hcnt, id, rank); }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SCAT_AGG_SLOTS; k += 1024) if (hkey[k] >= 0) hbase[k] = atomicAdd(&cur[hkey[k]], hcnt[k]);
    __syncthreads();
    if (id >= 0) { const int slot = hbase[h] + rank; sid[slot] = id; spos[slot] = concat ? i : pos; }
}

int sbr_scatter_lds_ids() { return SCAT_LDS_IDS; }

hipError_t launch_scatter_sort(hipStream_t s, const int* X, const int* len, int T, int Bp, int F, int n_ids, int* cnt,
                               int* offs, int* cur, int* sid, int* spos, int concat, int tch, int n_tchunks, const SbrTChunks* bounds,
                               int* cnt_zero_n) {
    const int ipc = n_ids;                          // ids per time chunk
    const SbrTChunks tc = bounds ? *bounds : SbrTChunks{};      // (no bounds: plain keys, n = 0)
    if (tch > 0) {
        n_ids *= n_tchunks;                         // key space
        if (n_ids > SCAT_LDS_IDS || tc.n != n_tchunks || tc.n > SBR_TCHUNKS_MAX || tc.lo[0] != 0 || tc.lo[tc.n] < T) return hipErrorInvalidValue;
    }
    // cnt_zero_n: how many leading counters the previous user of `cnt` left at zero (the LDS-path scan clears what it reads)
    if (!(cnt_zero_n && *cnt_zero_n >= n_ids)) {
        hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n_ids * sizeof(int), s);
        if (e != hipSuccess) return e;
    }
    if (cnt_zero_n) *cnt_zero_n = n_ids <= SCAT_LDS_IDS ? n_ids : 0;
    const int total = T * Bp * F;
    if (n_ids <= SCAT_LDS_IDS) {
        const int per_block = 4096;
        const int grid = (total + per_block - 1) / per_block;
        const size_t lds = (size_t)n_ids * sizeof(int);
        SBR_DYN_LDS(scat_count_lds_kernel, lds);
        SBR_DYN_LDS(scat_fill_lds_kernel, lds);
        scat_count_lds_kernel<<<grid, SCAT_BLOCK, lds, s>>>(X, len, T, Bp, F, n_ids, per_block, cnt, tc, ipc);
        SBR_DYN_LDS(scat_scan_kernel<true>, lds);
        scat_scan_kernel<true><<<1, 1024, lds, s>>>(cnt, n_ids, offs, cur);
        scat_fill_lds_kernel<<<grid, SCAT_BLOCK, lds, s>>>(X, len, T, Bp, F, n_ids, per_block, cur, sid, spos, concat, tc, ipc);
    } else {
        const int agrid = (total + 1023) / 1024;
        scat_count_agg_kernel<<<agrid, 1024, 0, s>>>(X, len, T, Bp, F, cnt);
        const int nb = (n_ids + SCAN_BLK - 1) / SCAN_BLK;
        if (nb <= 1) scat_scan_kernel<false><<<1, 1024, 0, s>>>(cnt, n_ids, offs, cur);
        else {      // block totals in cur[0 .. nb) (rewritten by the add), their prefixes in cnt[0 .. nb) (not read any more)
            scat_scan_local_kernel<<<nb, 1024, 0, s>>>(cnt, n_ids, offs, cur);
            scat_scan_totals_kernel<<<1, 1024, 0, s>>>(cur, nb, cnt, offs + n_ids);
            scat_scan_add_kernel<<<nb, 1024, 0, s>>>(cnt, n_ids, offs, cur);
        }
        scat_fill_agg_kernel<<<agrid, 1024, 0, s>>>(X, len, T, Bp, F, cur, sid, spos, concat);
    }
    return hipGetLastError();
}

#define SCAT_FLY 8     // rows in flight per wave
// SCAT_CHUNK sorted entries per wave: 64 puts 800 waves on the chip for C2's 51 200 entries (200 workgroups, one wave per
// SIMD: latency-bound, 1.6 TB/s of row reads); smaller chunks trade more seam atomics for memory-level parallelism
// (SBR_SCAT_CHUNK = 16 / 32 / 64).
// key_lo > 0 or ACC: the launch covers the sorted entries of the keys [key_lo, key_lo + n_ids) only (one time chunk of the
// time-chunked sort, row id = key - key_lo) and ADDS to rows earlier launches of the same stream have written.  (No launch asks for
// either any more: <4 | 8 | 16, 32> and the polling <1 | 2 | 4, 32, true, true> with key_lo = 0, their symbols and code as profiled.)
// POLL (overlapped step tail): ONE launch over all time chunks beside the running BPTT chain.  n_ids = ids per time chunk,
// keys = chunk * n_ids + id.  Waves take the sorted entries from the far end (late time steps are complete first); a wave
// waits (one lane polls poll.done, bounded) until the chain has left the time chunk of its FIRST entry -- the lowest of the
// wave, the order is ascending -- takes an agent-scope acquire, and adds its row sums with float atomics: an id may occur
// in every chunk, and chunks finish in different waves.
template <int NV, int SCAT_CHUNK, bool ACC = false, bool POLL = false>
__global__ void __launch_bounds__(256) scat_reduce_kernel(const f32x4* __restrict__ dxt, const int* __restrict__ sid,
                                                          const int* __restrict__ spos, const int* __restrict__ offs,
                                                          int n_ids, float* __restrict__ dWin, int R4, int Bp, int key_lo = 0,
                                                          int n_tchunks = 1, SbrTChunks tch = SbrTChunks(), SbrPoll poll = SbrPoll()) {
    // rows in flight per wave: narrow rows (NV = 1: at most 256 floats, C1's are 128) are latency, not bytes -- 16 of them
    constexpr int FLY = (NV == 1 && !POLL) ? 16 : SCAT_FLY;
    const int lane = threadIdx.x & 63;
    const int wave_global = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    const int total = offs[POLL ? n_ids * n_tchunks : key_lo + n_ids];
    // POLL: key_lo = the first key this launch takes (time chunk 0 -- the one the chain completes last -- is left to a launch
    // of its own behind the chain when key_lo = n_ids: see sbr_backward_recurrent)
    const int e_lo = POLL ? offs[key_lo] : 0;
    // POLL: the entries of the time chunks the chain completes LAST (chunks < poll.n_small: the last ~10 time steps with the
    // geometric bounds) are cut into SHORT pieces of SCAT_SHORT entries: what is left at the chain's end is then one round of
    // eight rows per wave instead of a 32-entry walk (four rounds and up to 32 flushes: 30 - 35 us behind the chain,
    // profiles/round3_f_timeline.txt)
    constexpr int SCAT_SHORT = 8;
    const int e_mid = POLL ? max(e_lo, min(total, offs[min(poll.n_small, n_tchunks) * n_ids])) : 0;
    const int nchA = POLL ? (total - e_mid + SCAT_CHUNK - 1) / SCAT_CHUNK : 0, nchB = POLL ? (e_mid - e_lo + SCAT_SHORT - 1) / SCAT_SHORT : 0;
    // POLL: a bounded number of waves (the launch must leave the chip to the GEMM that runs beside it) walks the sorted
    // entries from the far end, wave-chunk it, it + n_waves, ...
    for (int it = wave_global; ; it += n_waves) {
    int base, cnt;
    if (POLL) {
        if (it >= nchA + nchB) break;
        if (it < nchA) { base = e_mid + (nchA - 1 - it) * SCAT_CHUNK; cnt = min(SCAT_CHUNK, total - base); }
        else { base = e_lo + (nchB - 1 - (it - nchA)) * SCAT_SHORT; cnt = min(SCAT_SHORT, e_mid - base); }
    } else {
        base = offs[key_lo] + wave_global * SCAT_CHUNK;
        if (base >= total) return;
        cnt = min(SCAT_CHUNK, total - base);
    }
    const int lim = base + cnt;
    const int e = base + (lane & (SCAT_CHUNK - 1));
    const int my_id = e < lim ? sid[e] : -1;
    const int my_pos = e < lim ? spos[e] : 0;
    if (POLL) {
        const int t_need = tch.lo[min(__shfl(my_id, 0) / n_ids, SBR_TCHUNKS_MAX)];
        if (lane == 0) {
            const unsigned long long t0 = wall_clock64();
            const int* mine = poll.done + ((blockIdx.x + 16) & (SBR_DONE_COPIES - 1)) * SBR_DONE_STRIDE;
            for (;;) {
                const int v = __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((v >> 12) == poll.epoch && (v & 0xfff) <= t_need) break;
                if (wall_clock64() - t0 > SBR_POLL_TICKS) { atomicOr(poll.fault, 8); break; }
                poll_sleep((v >> 12) == poll.epoch ? (v & 0xfff) - t_need : 64);
            }
        }
        // (no acquire fence: on gfx950 that is an invalidate of the XCD's whole L2, ~15 000 cycles, for every released wave -- the
        // rows the chain wrote are read with sc1 loads below instead; sbr_gemm_x6.hip x6_poll_wait)
        __builtin_amdgcn_wave_barrier();
        if (poll.trace && lane == 0) {
            const int k = min((it - wave_global) / n_waves, 3);
            poll.trace[8192 + (wave_global * 4 + k) * 2] = wall_clock64();
        }
    }
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
    int cur_id = __shfl(my_id, 0);
#ifndef SCAT_DEBUG_NOFLUSH
#define SCAT_DEBUG_NOFLUSH 0      // 1 (tools/probes/variant_build.sh): the polling launch adds nothing -- WRONG gradients, for timing what its atomics cost
#endif
    auto flush = [&](int key) {
        if (POLL && SCAT_DEBUG_NOFLUSH) return;
        const bool owned = !POLL && offs[key] >= base && offs[key + 1] <= base + cnt;    // whole segment inside this chunk
        const int id = POLL ? key % n_ids : key - key_lo;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int f4 = lane + 64 * v;
            if (f4 < R4) {
                float* dst = dWin + ((size_t)id * R4 + f4) * 4;
                if (owned) { if (ACC) *(f32x4*)dst += acc[v]; else *(f32x4*)dst = acc[v]; }
                else { atomicAdd(dst, acc[v][0]); atomicAdd(dst + 1, acc[v][1]); atomicAdd(dst + 2, acc[v][2]); atomicAdd(dst + 3, acc[v][3]); }
            }
            acc[v] = f32x4{0, 0, 0, 0};
        }
    };
    for (int i = 0; i < cnt; i += FLY) {
        f32x4 val[FLY][NV];
        int ids[FLY];
#pragma unroll
        for (int u = 0; u < FLY; ++u) {                 // rows in flight
            const int ii = min(i + u, cnt - 1);
            ids[u] = __shfl(my_id, ii);
            const size_t pos = (size_t)__shfl(my_pos, ii);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int f4 = lane + 64 * v;
                if constexpr (POLL)      // (lanes past the row load its last piece: no branch around the asm; zeroed once landed)
                    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(val[u][v]) : "v"(dxt + pos * R4 + min(f4, R4 - 1)) : "memory");
                else val[u][v] = f4 < R4 ? dxt[pos * R4 + f4] : f32x4{0, 0, 0, 0};
            }
        }
        if constexpr (POLL) {      // (the loads above are invisible to the compiler's waitcnt insertion)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int u = 0; u < FLY; ++u)
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    asm volatile("" : "+v"(val[u][v]));
                    if (lane + 64 * v >= R4) val[u][v] = f32x4{0, 0, 0, 0};
                }
        }
#pragma unroll
        for (int u = 0; u < FLY; ++u) {
            if (i + u < cnt) {                                 // wave-uniform
                if (ids[u] != cur_id) { flush(cur_id); cur_id = ids[u]; }
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
            }
        }
    }
    flush(cur_id);
    if (POLL && poll.trace && lane == 0) {
        const int k = min((it - wave_global) / n_waves, 3);
        poll.trace[8192 + (wave_global * 4 + k) * 2 + 1] = wall_clock64();
    }
    if (!POLL) break;
    }
}

hipError_t launch_scatter_reduce_poll(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs,
                                      int n_ids, int n_tchunks, int max_entries, int GHp, int Bp, const SbrPoll& poll_in,
                                      const SbrTChunks& tc, int short_chunks, bool fence_on, const ScatPlan& plan) {
    SbrPoll poll = poll_in;
    poll.n_small = std::max(0, std::min(short_chunks, n_tchunks));      // (the field counts the GEMM's short slabs there; here: time chunks cut short)

    const int R4 = GHp / 4, nv = plan.poll_nv;
    const int wgs = 128;   // (round 3: 128 with the short pieces; 64 before)
    const int grid = std::max(1, std::min(wgs, ((max_entries + 7) / 8 + 3) / 4));
    // (the LDS this launch asks for is a FENCE, not storage: with it a workgroup does not fit beside the BPTT chain's, which claims
    // 124 KB of its CU's 160 for the same purpose -- sbr_rec_p.hip launch_bwd_p)
    const size_t fence = fence_on ? (size_t)40 * 1024 : 0;
#define SRP(NV) scat_reduce_kernel<NV, 32, true, true><<<grid, 256, fence, s>>>((const f32x4*)dxt, sid, spos, offs, n_ids, dWin, R4, Bp, 0, n_tchunks, tc, poll)
    if (nv == 1) SRP(1); else if (nv == 2) SRP(2); else if (nv == 4) SRP(4); else return hipErrorInvalidValue;      // (0: rows beyond 1024 floats)
#undef SRP
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Overlapped step tail, round 3: the scatter-add WITHOUT one global atomic per piece and row.
// The polling launch above adds every piece's row sums to dW_in with float atomics: an id occurs in every time chunk and its
// entries are cut into pieces, ~10 000 flushes of 384 floats per C2 step.  On gfx950 agent-scope atomics are executed by the
// memory side, and 4 M of them beside the chain cost the chain 13 us, the polling GEMM's last slabs 10 us and this launch's
// own end 17 us (profiles/round3_w_trace.txt: the same step with the flush removed).
// Here a workgroup OWNS a range of ids: it walks the time chunks in the order the chain releases them, adds the rows of its
// ids' entries into accumulators in LDS (ds_add_f32), and stores each row ONCE when the chain has ended.  Ranges are cut in
// COST space, cost(id) = max(entries of id over all chunks, floor): unit u owns [u Q, (u + 1) Q) of the running sum P, so that
// units are balanced in entries and hold at most Q / floor + 2 ids (the LDS rows); an id that straddles a cut -- every hot id
// does -- is shared: in EVERY chunk each sharing unit takes the same fraction of that id's entries (the cut is uniform in
// time, so nobody is left with only the last time steps), and only those rows, at most two per unit, end in global atomics.
// In the time-chunked sort the entries of a unit in one chunk are one contiguous range of the sorted array.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) scat_cost_scan_kernel(const int* __restrict__ offs, int n_ids, int n_tchunks, int floor_cost,
                                                              int* __restrict__ P) {
    __shared__ int part[1024];
    const int per = (n_ids + 1023) / 1024, lo = threadIdx.x * per, hi = min(n_ids, lo + per);
    int sum = 0;
    for (int id = lo; id < hi; ++id) {
        int tot = 0;
        for (int c = 0; c < n_tchunks; ++c) tot += offs[c * n_ids + id + 1] - offs[c * n_ids + id];
        sum += max(tot, floor_cost);
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;                               // exclusive
    for (int id = lo; id < hi; ++id) {
        int tot = 0;
        for (int c = 0; c < n_tchunks; ++c) tot += offs[c * n_ids + id + 1] - offs[c * n_ids + id];
        P[id] = run;
        run += max(tot, floor_cost);
    }
    if (threadIdx.x == 1023) P[n_ids] = part[1023];
}

template <int NV>
__global__ void __launch_bounds__(256) scat_lds_kernel(const f32x4* __restrict__ dxt, const int* __restrict__ sid, const int* __restrict__ spos,
                                                       const int* __restrict__ offs, const int* __restrict__ P, int n_ids, int n_tchunks,
                                                       float* __restrict__ dWin, int R4, SbrTChunks tch, SbrPoll poll, int rows_lds,
                                                       int monitor, int t_lo) {
    // monitor != 0: workgroup 0 -- the first on the chip -- is the tail's MONITOR (tail_monitor_loop) and nothing else; the
    // units are workgroups 1 .. gridDim.x - 1.  No stream of its own then -- hardware queues are few (a FOURTH side stream for
    // the monitor halved the throughput of everything, profiles/round3_A_variants.txt), and this launch is the first of the
    // tail on its stream anyway.
    if (monitor && blockIdx.x == 0) { tail_monitor_loop(poll, t_lo); return; }
    const int unit = (int)blockIdx.x - (monitor ? 1 : 0);
    extern __shared__ float rows[];                                  // [rows_lds][4][R4]: component-major rows (no bank conflicts)
    __shared__ int s_meta[4];
    __shared__ int s_e0[SBR_TCHUNKS_MAX + 1], s_e1[SBR_TCHUNKS_MAX + 1], s_kf[SBR_TCHUNKS_MAX + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = P[n_ids], U = (int)gridDim.x - (monitor ? 1 : 0), Q = (total + U - 1) / U;
    const int lo = unit * Q, hi = min(total, lo + Q);
    if (lo >= hi) return;
    if (tid == 0) {                                                  // the ids of P that hold cost positions lo and hi - 1
        int a = 0, b = n_ids - 1;
        while (a < b) { const int m = (a + b + 1) >> 1; if (P[m] <= lo) a = m; else b = m - 1; }
        s_meta[0] = a;
        b = n_ids - 1;
        while (a < b) { const int m = (a + b + 1) >> 1; if (P[m] <= hi - 1) a = m; else b = m - 1; }
        s_meta[1] = a;
    }
    __syncthreads();
    const int id_first = s_meta[0], id_last = s_meta[1];
    int n_rows = id_last - id_first + 1;
    if (n_rows > rows_lds) { if (tid == 0) atomicOr(poll.fault, 16); n_rows = rows_lds; }      // (cannot happen: launch_scatter_lds_poll sizes rows_lds)
    const long num0 = lo - P[id_first], den0 = P[id_first + 1] - P[id_first];
    const long num1 = hi - P[id_last], den1 = P[id_last + 1] - P[id_last];
    const int RW = 4 * R4;
    for (int i = tid; i < n_rows * RW; i += 256) rows[i] = 0.f;
    if (tid < n_tchunks) {                                           // this unit's range of the sorted entries in every time chunk
        const int kf = tid * n_ids + id_first, kl = tid * n_ids + id_last;
        const int b0 = offs[kf], b1 = offs[kl];
        s_e0[tid] = b0 + (int)(num0 * (offs[kf + 1] - b0) / den0);
        s_e1[tid] = b1 + (int)(num1 * (offs[kl + 1] - b1) / den1);
        s_kf[tid] = kf;
    }
    __syncthreads();
    int seen = 0xfff;
    const int* mine = poll.done + ((unit + 16) & (SBR_DONE_COPIES - 1)) * SBR_DONE_STRIDE;
    for (int c = n_tchunks - 1; c >= 0; --c) {
        const int kf = s_kf[c], e0 = s_e0[c], e1 = s_e1[c];
        if (e0 >= e1) continue;                                      // (uniform)
        const int t_need = tch.lo[c];
        // the first strip's keys and positions (written by the sort, long complete) are on their way while the workgroup waits
        const int base_0 = e0 + wave * SCAT_FLY, cnt_0 = min(SCAT_FLY, e1 - base_0);
        int key_0 = lane < cnt_0 ? sid[base_0 + lane] : -1;
        int pos_0 = lane < cnt_0 ? spos[base_0 + lane] : 0;
        if (seen > t_need) {                                         // the chain has not left this time chunk yet, as far as this workgroup knows
            if (tid == 0) {
                const unsigned long long t0 = wall_clock64();
                for (;;) {
                    const int v = __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((v >> 12) == poll.epoch && (v & 0xfff) <= t_need) { s_meta[2] = v & 0xfff; break; }
                    if (wall_clock64() - t0 > SBR_POLL_TICKS) { atomicOr(poll.fault, 8); s_meta[2] = 0; break; }
                    poll_sleep((v >> 12) == poll.epoch ? (v & 0xfff) - t_need : 64);
                }
            }
            __syncthreads();
            seen = s_meta[2];
            __syncthreads();
        }
        if (poll.trace && tid == 0) poll.trace[8192 + (unit * 16 + c) * 2] = wall_clock64();
        // strips of SCAT_FLY entries, round-robin over the four waves; rows read with sc1 loads (no acquire fence: scat_reduce_kernel)
        for (int base = base_0; base < e1; base += 4 * SCAT_FLY) {
            const int cnt = min(SCAT_FLY, e1 - base);
            const int my_key = base == base_0 ? key_0 : (lane < cnt ? sid[base + lane] : -1);
            const int my_pos = base == base_0 ? pos_0 : (lane < cnt ? spos[base + lane] : 0);
            f32x4 val[SCAT_FLY][NV];
#pragma unroll
            for (int u = 0; u < SCAT_FLY; ++u) {
                const size_t pos = (size_t)__shfl(my_pos, min(u, cnt - 1));
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(val[u][v]) : "v"(dxt + pos * R4 + min(lane + 64 * v, R4 - 1)) : "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int u = 0; u < SCAT_FLY; ++u)
#pragma unroll
                for (int v = 0; v < NV; ++v) asm volatile("" : "+v"(val[u][v]));
            f32x4 acc[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
            int cur = __shfl(my_key, 0);
            auto flush = [&](int key) {
                float* r = rows + (size_t)min(key - kf, n_rows - 1) * RW;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int f4 = lane + 64 * v;
                    if (f4 < R4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) atomicAdd(r + e * R4 + f4, acc[v][e]);
                    }
                    acc[v] = f32x4{0, 0, 0, 0};
                }
            };
#pragma unroll
            for (int u = 0; u < SCAT_FLY; ++u) {
                if (u < cnt) {                                       // (uniform)
                    const int k = __shfl(my_key, u);
                    if (k != cur) { flush(cur); cur = k; }
#pragma unroll
                    for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
                }
            }
            flush(cur);
        }
        if (poll.trace && tid == 0) poll.trace[8192 + (unit * 16 + c) * 2 + 1] = wall_clock64();
    }
    __syncthreads();
    // one store per row; the (at most two) rows shared with the neighbouring units go by atomics
    for (int r = wave; r < n_rows; r += 4) {
        const bool shared = (r == 0 && num0 > 0) || (r == n_rows - 1 && num1 < den1);
        const float* src = rows + (size_t)r * RW;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int f4 = lane + 64 * v;
            f32x4 x = f32x4{0, 0, 0, 0};
            if (f4 < R4) { x[0] = src[f4]; x[1] = src[R4 + f4]; x[2] = src[2 * R4 + f4]; x[3] = src[3 * R4 + f4]; }
            const bool nz = x[0] != 0.f || x[1] != 0.f || x[2] != 0.f || x[3] != 0.f;
            if (f4 < R4 && nz) {
                float* dst = dWin + ((size_t)(id_first + r) * R4 + f4) * 4;
                if (shared) { atomicAdd(dst, x[0]); atomicAdd(dst + 1, x[1]); atomicAdd(dst + 2, x[2]); atomicAdd(dst + 3, x[3]); }
                else *(f32x4*)dst = x;
            }
        }
    }
    if (poll.trace && tid == 0) poll.trace[8192 + (unit * 16 + 15) * 2] = wall_clock64();
}

// behind the time-chunked sort (same stream) where the tail's form is SCAT_LDS: the running cost P[0 .. n_ids] of the ids
hipError_t launch_scatter_cost_scan(hipStream_t s, const int* offs, int* P, int n_ids, int n_tchunks, const ScatPlan& plan) {
    scat_cost_scan_kernel<<<1, 1024, 0, s>>>(offs, n_ids, n_tchunks, plan.floor_cost, P);
    return hipGetLastError();
}
hipError_t launch_scatter_lds_poll(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs, const int* P,
                                   int n_ids, int n_tchunks, int GHp, const SbrPoll& poll, const SbrTChunks& bounds,
                                   int units, const ScatPlan& plan, bool monitor, int t_lo) {
    const int R4 = GHp / 4, rows_lds = plan.rows_lds, grid = units + (monitor ? 1 : 0), mon = monitor ? 1 : 0;
    const size_t lds = (size_t)rows_lds * GHp * sizeof(float);
    if (plan.lds_nv == 1) { SBR_DYN_LDS(scat_lds_kernel<1>, lds); scat_lds_kernel<1><<<grid, 256, lds, s>>>((const f32x4*)dxt, sid, spos, offs, P, n_ids, n_tchunks, dWin, R4, bounds, poll, rows_lds, mon, t_lo); }
    else if (plan.lds_nv == 2) { SBR_DYN_LDS(scat_lds_kernel<2>, lds); scat_lds_kernel<2><<<grid, 256, lds, s>>>((const f32x4*)dxt, sid, spos, offs, P, n_ids, n_tchunks, dWin, R4, bounds, poll, rows_lds, mon, t_lo); }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Wide rows (G*Hp >= 512 floats: the cluster layers, C3 / C4 / C5): segment-parallel scatter-add, no atomics on rows, fixed order.
// The wave-per-32-entries kernel above adds every segment that is not wholly inside a chunk with float atomics; with Zipf ids
// the hot rows' segments span hundreds of chunks and their adds serialise at the memory side (C4: 199 us for 210 MB of rows,
// 1 TB/s; C5 571 us) -- while most segments of a large catalogue are ONE entry, i.e. a row copy.  Three launches:
//   heads   one wave per sorted entry; a wave whose entry is not the first of its id leaves at once.  The head of a segment of
//           <= SCATW_SHORT entries sums its rows (SCATW_FLY in flight, 16 bytes per lane and piece) and stores dW_in[id]; the head
//           of a longer segment claims ceil(len / SCATW_SHORT) slots of the partial-row slab (one atomic on a counter) and files
//           (id, first entry, length, first slot) in the list of long segments
//   pieces  one workgroup per slab slot: the SCATW_SHORT entries of that piece -> the slot's partial row
//   merge   one workgroup per long segment: its slots summed in order -> dW_in[id]
// Every row has one writer and a fixed summation order (the slot numbers depend on which head reached the counter first, the sums
// do not): the gradient is bit-reproducible.  A long segment claims ceil(len / 64) <= len / 64 + 1 slots and has more than 64 entries:
// at most entries / 64 + entries / 65 slots and entries / 65 long segments exist (sbr_scatter_wide_slots; the launcher refuses a
// smaller slab -- round 4 sized it entries / 64 + 2, which segments of 65 .. 127 entries could overrun).
// (sparse_lstm.py:368: the AdvancedIncSubtensor the reference's backward builds.)
// ---------------------------------------------------------------------------------------
#define SCATW_SHORT 64
#define SCATW_FLY 4
struct ScatLong { int id, first, len, slot; };
template <int NV>
__global__ void __launch_bounds__(256) scat_heads_kernel(const f32x4* __restrict__ dxt, const int* __restrict__ sid,
                                                         const int* __restrict__ spos, const int* __restrict__ offs, int n_ids,
                                                         float* __restrict__ dWin, int R4, int* __restrict__ counters,
                                                         ScatLong* __restrict__ longs) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), total = offs[n_ids];
    if (e >= total) return;
    const int id = sid[e];
    if (e > 0 && sid[e - 1] == id) return;               // not the head of its segment
    const int len = offs[id + 1] - offs[id];
    if (len > SCATW_SHORT) {
        if (lane == 0) {
            const int np = (len + SCATW_SHORT - 1) / SCATW_SHORT;
            const int slot = atomicAdd(counters, np), k = atomicAdd(counters + 1, 1);
            longs[k] = ScatLong{id, e, len, slot};
        }
        return;
    }
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
    for (int i = 0; i < len; i += SCATW_FLY) {
        f32x4 val[SCATW_FLY][NV];
#pragma unroll
        for (int u = 0; u < SCATW_FLY; ++u) {
            if (i + u < len) {                           // uniform (most segments of a large catalogue are one entry: a row copy)
                const size_t pos = (size_t)spos[e + i + u];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int f4 = lane + 64 * v;
                    val[u][v] = f4 < R4 ? dxt[pos * R4 + f4] : f32x4{0, 0, 0, 0};
                }
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) val[u][v] = f32x4{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int u = 0; u < SCATW_FLY; ++u)
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) { const int f4 = lane + 64 * v; if (f4 < R4) ((f32x4*)dWin)[(size_t)id * R4 + f4] = acc[v]; }
}

// one workgroup per slab slot: blockIdx.x = slot; the segment that owns it is found by a scan of the (short) list
template <int NV>
__global__ void __launch_bounds__(256) scat_pieces_kernel(const f32x4* __restrict__ dxt, const int* __restrict__ spos,
                                                          const int* __restrict__ counters, const ScatLong* __restrict__ longs,
                                                          f32x4* __restrict__ part, int R4) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (slot >= counters[0]) return;
    const int nl = counters[1];
    __shared__ int s_seg;
    if (tid == 0) s_seg = -1;
    __syncthreads();
    for (int k = tid; k < nl; k += 256) {
        const ScatLong L = longs[k];
        if (slot >= L.slot && slot < L.slot + (L.len + SCATW_SHORT - 1) / SCATW_SHORT) s_seg = k;
    }
    __syncthreads();
    if (s_seg < 0) return;
    const ScatLong L = longs[s_seg];
    const int lo = L.first + (slot - L.slot) * SCATW_SHORT, hi = min(L.first + L.len, lo + SCATW_SHORT);
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
    for (int i = lo; i < hi; i += 8) {
        f32x4 val[8][NV];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t pos = (size_t)spos[min(i + u, hi - 1)];
#pragma unroll
            for (int v = 0; v < NV; ++v) { const int f4 = tid + 256 * v; val[u][v] = f4 < R4 ? dxt[pos * R4 + f4] : f32x4{0, 0, 0, 0}; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i + u < hi) {
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
            }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) { const int f4 = tid + 256 * v; if (f4 < R4) part[(size_t)slot * R4 + f4] = acc[v]; }
}

template <int NV>
__global__ void __launch_bounds__(256) scat_long_merge_kernel(const f32x4* __restrict__ part, const int* __restrict__ counters,
                                                              const ScatLong* __restrict__ longs, float* __restrict__ dWin, int R4) {
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= counters[1]) return;
    const ScatLong L = longs[k];
    const int np = (L.len + SCATW_SHORT - 1) / SCATW_SHORT;
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
    for (int p0 = 0; p0 < np; p0 += 8) {
        f32x4 val[8][NV];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t sl = (size_t)(L.slot + min(p0 + u, np - 1));
#pragma unroll
            for (int v = 0; v < NV; ++v) { const int f4 = tid + 256 * v; val[u][v] = f4 < R4 ? part[sl * R4 + f4] : f32x4{0, 0, 0, 0}; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (p0 + u < np) {
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
            }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) { const int f4 = tid + 256 * v; if (f4 < R4) ((f32x4*)dWin)[(size_t)L.id * R4 + f4] = acc[v]; }
}

// part: n_slots * GHp floats (n_slots >= sbr_scatter_wide_slots(max_entries): the plan has checked it); aux: 2 counters + n_slots
// ScatLong records (ints)
hipError_t launch_scatter_wide(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs, int n_ids,
                               int max_entries, int GHp, float* part, int* aux, int n_slots, const ScatPlan& plan) {
    const int R4 = GHp / 4, nvw = plan.wide_nvw;
    if (hipMemsetAsync(aux, 0, 2 * sizeof(int), s) != hipSuccess) return hipGetLastError();
    int* counters = aux; ScatLong* longs = (ScatLong*)(aux + 4);
    const int gh = (max_entries + 3) / 4;
#define SW(NVW, NVB) do { \
        scat_heads_kernel<NVW><<<gh, 256, 0, s>>>((const f32x4*)dxt, sid, spos, offs, n_ids, dWin, R4, counters, longs); \
        scat_pieces_kernel<NVB><<<n_slots, 256, 0, s>>>((const f32x4*)dxt, spos, counters, longs, (f32x4*)part, R4); \
        scat_long_merge_kernel<NVB><<<n_slots, 256, 0, s>>>((const f32x4*)part, counters, longs, dWin, R4); } while (0)
    if (nvw == 2) SW(2, 1); else if (nvw == 4) SW(4, 1); else if (nvw == 8) SW(8, 2); else return hipErrorInvalidValue;      // (.wide_nvb goes with it)
#undef SW
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Wide rows, form 1 ("range" scatter-add; default for G*Hp <= 1024: C3 / C4): two passes, no atomics, fixed order.
// (Form 2, the segment-parallel kernels above, is the faster one ALONE -- 100 against 164 us at C4 -- but this one keeps its pace beside the
// weight-gradient GEMM it shares the chip with after the BPTT chain: 512 persistent workgroups instead of 12 800 short ones; measured
// C4 1.315 ms with it against 1.372 with form 2 on the same stream and 1.370 with form 2 alone in front of the GEMM: profiles/round4_variants_wide.txt.)
// The wave-per-32-entries kernel above adds every segment that is not wholly inside a chunk with float atomics; with Zipf ids
// the hot rows' segments span hundreds of chunks and their adds serialise at the memory side (C4: 199 us for 210 MB of rows,
// 1 TB/s; C5 571 us).  Here a workgroup owns a contiguous RANGE of the sorted entries, a thread owns one 16-byte piece of
// the row (a 1024-float row = one piece per thread: every row load is one fully coalesced 4 KB access, SCATR_FLY rows in
// flight), the range is walked once with the running sum in registers.  Segments inside the range are stored straight to
// dW_in; the range's FIRST and LAST segment -- the only ones another range can share -- go to a partial-row slab
// [range][2][row] with their ids beside them, and the merge pass (one workgroup per partial slot; the leader of a run of
// equal ids sums the run in slot order) writes those rows.  Every row has exactly one writer and a fixed summation order:
// the gradient is bit-reproducible.  (sparse_lstm.py:368: the AdvancedIncSubtensor the reference's backward builds.)
// ---------------------------------------------------------------------------------------
// (Round 6 measured a software-pipelined walk -- the range's (id, position) pairs staged in LDS, two register sets of SCATR_FLY rows
// alternating, the flushes counted out of its waits: ALONE on the chip 60.8 against 67.5 us at C4 (4.17 TB/s), but 194 against 112 us
// in the step, where it runs beside the weight-gradient GEMM: 80 registers instead of 48 halve what fits beside that launch's
// workgroups.  The two launches together are no faster than one after the other either way -- profiles/round6_variants.txt, calls d, e.)
#define SCATR_FLY 8
template <int NV>
__global__ void __launch_bounds__(256) scat_range_kernel(const f32x4* __restrict__ dxt, const int* __restrict__ sid,
                                                         const int* __restrict__ spos, const int* __restrict__ total_p,
                                                         float* __restrict__ dWin, int R4, f32x4* __restrict__ part,
                                                         int* __restrict__ part_id) {
    const int total = *total_p, nr = gridDim.x, w = blockIdx.x, tid = threadIdx.x;
    const int E = (total + nr - 1) / nr;
    const int lo = min(total, w * E), hi = min(total, lo + E);
    if (lo >= hi) { if (tid < 2) part_id[2 * w + tid] = -1; return; }
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
    const int first_id = sid[lo], last_id = sid[hi - 1];
    int cur = first_id;
    bool in_first = true;
    auto flush = [&](int id, bool last) {              // uniform arguments
        f32x4* dst = (in_first || last) ? part + ((size_t)(2 * w + (in_first ? 0 : 1)) * R4)
                                        : (f32x4*)dWin + (size_t)id * R4;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int f4 = tid + 256 * v;
            if (f4 < R4) dst[f4] = acc[v];
            acc[v] = f32x4{0, 0, 0, 0};
        }
        in_first = false;
    };
    for (int i = lo; i < hi; i += SCATR_FLY) {
        f32x4 val[SCATR_FLY][NV];
        int ids[SCATR_FLY];
#pragma unroll
        for (int u = 0; u < SCATR_FLY; ++u) {
            const int e = min(i + u, hi - 1);
            ids[u] = sid[e];
            const size_t pos = (size_t)spos[e];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int f4 = tid + 256 * v;
                val[u][v] = f4 < R4 ? dxt[pos * R4 + f4] : f32x4{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int u = 0; u < SCATR_FLY; ++u) {
            if (i + u < hi) {                            // uniform
                const int id = __builtin_amdgcn_readfirstlane(ids[u]);
                if (id != cur) { flush(cur, false); cur = id; }
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
            }
        }
    }
    const bool single = in_first;                        // the whole range is one segment: it went (goes) to slot 0
    flush(cur, true);
    if (tid == 0) { part_id[2 * w] = first_id; part_id[2 * w + 1] = single ? -1 : last_id; }
}

// The merge of the shared first / last segments.  A hot id's run spans many slots (Zipf: item 0 is ~9 % of C4's entries = ~90 slots of
// 512 ranges); the leader summed them one dependent load after the other (47 us at C4).  Now: the run's end first (ids only), then
// its rows SCATR_FLY at a time.
template <int NV>
__global__ void __launch_bounds__(256) scat_range_merge_kernel(const f32x4* __restrict__ part, const int* __restrict__ part_id,
                                                               int n_slots, float* __restrict__ dWin, int R4) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int id = part_id[p];
    if (id < 0) return;
    // previous slot that holds a row: the last segment of the range in front, or (that range being one segment) its first
    int prev = -2;
    if (p & 1) prev = part_id[p - 1];
    else if (p >= 2) prev = part_id[p - 1] >= 0 ? part_id[p - 1] : part_id[p - 2];
    if (prev == id) return;                              // not the leader of its run
    int qend = p + 1;                                    // one past the run's last slot (empty slots inside a run are skipped below)
    while (qend < n_slots) { const int iq = part_id[qend]; if (iq >= 0 && iq != id) break; ++qend; }
    f32x4 acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) { const int f4 = tid + 256 * v; acc[v] = f4 < R4 ? part[(size_t)p * R4 + f4] : f32x4{0, 0, 0, 0}; }
    for (int q0 = p + 1; q0 < qend; q0 += SCATR_FLY) {
        f32x4 val[SCATR_FLY][NV];
#pragma unroll
        for (int u = 0; u < SCATR_FLY; ++u) {
            const int q = min(q0 + u, qend - 1);
            const bool live = q0 + u < qend && part_id[q] == id;       // uniform
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int f4 = tid + 256 * v;
                val[u][v] = (live && f4 < R4) ? part[(size_t)q * R4 + f4] : f32x4{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int u = 0; u < SCATR_FLY; ++u)              // slot order: the sum is reproducible
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) { const int f4 = tid + 256 * v; if (f4 < R4) ((f32x4*)dWin)[(size_t)id * R4 + f4] = acc[v]; }
}

// part: n_ranges * 2 * GHp floats, part_id: n_ranges * 2 ints
hipError_t launch_scatter_range(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs, int n_ids,
                                int GHp, float* part, int* part_id, int n_ranges, const ScatPlan& plan) {
    const int R4 = GHp / 4, nv = plan.range_nv;
    const int* total_p = offs + n_ids;
#define SRG(NV) do { scat_range_kernel<NV><<<n_ranges, 256, 0, s>>>((const f32x4*)dxt, sid, spos, total_p, dWin, R4, (f32x4*)part, part_id); \
                     scat_range_merge_kernel<NV><<<2 * n_ranges, 256, 0, s>>>((const f32x4*)part, part_id, 2 * n_ranges, dWin, R4); } while (0)
    if (nv == 1) SRG(1); else if (nv == 2) SRG(2); else if (nv == 4) SRG(4); else return hipErrorInvalidValue;
#undef SRG
    return hipGetLastError();
}

// The plain scatter-add of rows up to 512 floats (round 6): scat_reduce_kernel's walk, 32 sorted entries per wave, with the partial rows
// of the segments that cross a wave's chunk COMBINED inside the workgroup before anything is added to memory.  A hot id spans many
// chunks, and every one of them used to add its partial row onto the same addresses with float atomics -- at C1 (3 706 ids, the hottest
// with thousands of the step's 51 200 entries) that serialisation was most of the launch (41 us for 26 MB).  Here the W waves of a
// workgroup take W consecutive chunks, leave at most two open partial rows each (the segment that began before the chunk, the one that
// goes on behind it) in LDS, and one wave adds up the runs of equal ids: a run that lies inside the workgroup's entries is STORED, only
// the runs that cross a workgroup boundary are added atomically -- W times fewer atomics on the hot rows.
template <int NV>
__global__ void __launch_bounds__(512) scat_reduce_comb_kernel(const f32x4* __restrict__ dxt, const int* __restrict__ sid,
                                                                              const int* __restrict__ spos, const int* __restrict__ offs,
                                                                              int n_ids, float* __restrict__ dWin, int R4) {
#ifndef COMB_CH
#define COMB_CH 32      // sorted entries per wave: 64 / 32 / 16 -> 29.3 / 21.5 / 22.6 us at C2 (profiles/round6_variants.txt, call y)
#endif
#ifndef COMB_FLY
#define COMB_FLY 8
#endif
    constexpr int CH = COMB_CH, FLY = NV >= 8 ? 2 : NV >= 4 ? 4 : COMB_FLY, W = 8;      // (wide rows: fewer in flight, the pieces stay near 64 registers)
    extern __shared__ __attribute__((aligned(16))) char comb_lds[];
    f32x4 (*slot)[NV * 64] = (f32x4 (*)[NV * 64])comb_lds;                         // [2 W][NV * 64]
    int* slot_id = (int*)(comb_lds + (size_t)2 * W * NV * 64 * sizeof(f32x4));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2 * W) slot_id[threadIdx.x] = -1;
    __syncthreads();
    const int total = offs[n_ids];
    const int wg_base = blockIdx.x * W * CH, wg_end = min(total, wg_base + W * CH);
    const int base = wg_base + wave * CH;
    // Whether a segment ends inside a chunk / a run inside the workgroup is read off the NEIGHBOURING entries' ids (the entries are sorted),
    // two loads per wave up front -- not off offs[key], offs[key + 1] at every flush: with a million ids those were two dependent trips to
    // HBM per distinct id of the chunk (C5: ~30 per wave), most of the launch.
    const int wg_prev = (wave == 0 && wg_base > 0 && wg_base < total) ? sid[wg_base - 1] : -1;
    const int wg_next = (wave == 0 && wg_end < total) ? sid[wg_end] : -1;
    auto row_out = [&](int key, const f32x4 (&a)[NV], bool store) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int f4 = lane + 64 * v;
            if (f4 < R4) {
                float* dst = dWin + ((size_t)key * R4 + f4) * 4;
                if (store) *(f32x4*)dst = a[v];
                else { atomicAdd(dst, a[v][0]); atomicAdd(dst + 1, a[v][1]); atomicAdd(dst + 2, a[v][2]); atomicAdd(dst + 3, a[v][3]); }
            }
        }
    };
    if (base < total) {
        const int cnt = min(CH, total - base);
        const int e = base + lane;
        const int my_id = lane < cnt ? sid[e] : -1;
        const int my_pos = lane < cnt ? spos[e] : 0;
        const int prev_id = base > 0 ? sid[base - 1] : -1, next_id = base + cnt < total ? sid[base + cnt] : -1;      // (uniform)
        f32x4 acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
        int cur_id = __shfl(my_id, 0);
        auto flush = [&](int key) {
            if (key != prev_id && key != next_id) row_out(key, acc, true);      // the whole segment inside this chunk
            else {
                const int sl = wave * 2 + (key == prev_id ? 0 : 1);             // began before the chunk | goes on behind it
#pragma unroll
                for (int v = 0; v < NV; ++v) slot[sl][lane + 64 * v] = acc[v];
                if (lane == 0) slot_id[sl] = key;
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = f32x4{0, 0, 0, 0};
        };
        for (int i = 0; i < cnt; i += FLY) {
            f32x4 val[FLY][NV];
            int ids[FLY];
#pragma unroll
            for (int u = 0; u < FLY; ++u) {
                const int ii = min(i + u, cnt - 1);
                ids[u] = __shfl(my_id, ii);
                const size_t pos = (size_t)__shfl(my_pos, ii);
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const int f4 = lane + 64 * v;
                    val[u][v] = f4 < R4 ? dxt[pos * R4 + f4] : f32x4{0, 0, 0, 0};
                }
            }
#pragma unroll
            for (int u = 0; u < FLY; ++u) {
                if (i + u < cnt) {                                 // wave-uniform
                    if (ids[u] != cur_id) { flush(cur_id); cur_id = ids[u]; }
#pragma unroll
                    for (int v = 0; v < NV; ++v) acc[v] += val[u][v];
                }
            }
        }
        flush(cur_id);
    }
    __syncthreads();
    if (wave == 0) {       // runs of equal ids among the open partial rows, in entry order
        int cur = -1;
        f32x4 sum[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) sum[v] = f32x4{0, 0, 0, 0};
        auto out = [&](int key) { row_out(key, sum, key != wg_prev && key != wg_next); };      // a run inside the workgroup's entries: stored
        for (int sl = 0; sl < 2 * W; ++sl) {
            const int id = slot_id[sl];                            // (uniform)
            if (id < 0) continue;
            if (id != cur) {
                if (cur >= 0) out(cur);
                cur = id;
#pragma unroll
                for (int v = 0; v < NV; ++v) sum[v] = f32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) sum[v] += slot[sl][lane + 64 * v];
        }
        if (cur >= 0) out(cur);
    }
}

// The recipe of the sorted segment reduce for rows of row_floats floats (ScatPlan.reduce; the embedding table's rows take it too).
// Rows whose 16-byte pieces fill 1, 2, 4 or 8 times a wave (up to 512 floats, 513 .. 1024, 1537 .. 2048): the combining form, 8 waves x
// 32 entries per workgroup (alone on the chip: C2's shape 43.4 -> 21.5 us, C1's 26.9 -> 14.8; C1's step 0.298 -> 0.286 ms:
// profiles/round6_variants.txt, call y).  Every other width up to 4096 floats: scat_reduce_kernel's walk, 32 entries per wave, on the
// next of its widths 4, 8, 16.  Wider rows have no kernel (nv = 0: the launch fails).
ScatReduce sbr_scat_reduce_recipe(int row_floats) {
    const int nv = (row_floats / 4 + 63) / 64;
    if (nv <= 2 || nv == 4 || nv == 8) return {nv, true};
    return {nv <= 4 ? 4 : nv <= 8 ? 8 : nv <= 16 ? 16 : 0, false};
}
hipError_t launch_scatter_reduce(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos,
                                 const int* offs, int n_ids, int max_entries, int GHp, int Bp, const ScatReduce& r) {
    const int R4 = GHp / 4;
    if (r.comb) {
        const int grid = (max_entries + 8 * COMB_CH - 1) / (8 * COMB_CH);
#define SRC(NV) do { const size_t lds = (size_t)16 * NV * 64 * sizeof(f32x4) + 64; SBR_DYN_LDS(scat_reduce_comb_kernel<NV>, lds); \
                     scat_reduce_comb_kernel<NV><<<grid, 512, lds, s>>>((const f32x4*)dxt, sid, spos, offs, n_ids, dWin, R4); } while (0)
        if (r.nv == 1) SRC(1); else if (r.nv == 2) SRC(2); else if (r.nv == 4) SRC(4); else SRC(8);
#undef SRC
        return hipGetLastError();
    }
    const int grid = ((max_entries + 31) / 32 + 3) / 4;
#define SR(NV) scat_reduce_kernel<NV, 32><<<grid, 256, 0, s>>>((const f32x4*)dxt, sid, spos, offs, n_ids, dWin, R4, Bp)
    if (r.nv == 4) SR(4); else if (r.nv == 8) SR(8); else if (r.nv == 16) SR(16); else return hipErrorInvalidValue;
#undef SR
    return hipGetLastError();
}

// triage fallback: per-element float atomics (SBR_FLAG_ATOMIC_SCATTER)
__global__ void scatter_rows_kernel(float* __restrict__ dWin, const f32x4* __restrict__ dxt, const int* __restrict__ X,
                                    const int* __restrict__ len, int T, int Bp, int F, int R4) {
    const size_t total = (size_t)T * Bp * R4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int f4 = (int)(i % R4);
        const size_t pos = i / R4;
        const int b = (int)(pos % Bp), t = (int)(pos / Bp);
        if (t >= len[b]) continue;
        const f32x4 v = dxt[i];
        const int* ids = X + ((size_t)b * T + t) * F;
        for (int f = 0; f < F; ++f) {
            float* dst = dWin + ((size_t)ids[f] * R4 + f4) * 4;
            atomicAdd(dst + 0, v[0]); atomicAdd(dst + 1, v[1]); atomicAdd(dst + 2, v[2]); atomicAdd(dst + 3, v[3]);
        }
    }
}

hipError_t launch_scatter_rows(hipStream_t s, float* dWin, const float* dxt, const int* X, const int* len, int T,
                               int Bp, int F, int GHp) {
    const int R4 = GHp / 4;
    const size_t total = (size_t)T * Bp * R4;
    const int grid = (int)min((size_t)256 * 16, (total + 255) / 256);
    scatter_rows_kernel<<<grid, 256, 0, s>>>(dWin, (const f32x4*)dxt, X, len, T, Bp, F, R4);
    return hipGetLastError();
}

// ScatPlan (sbr_common.h): the form of the scatter-add of layer 0's index-input gradient and its launch recipe, from values that are
// all fixed when the engine is created (sbr_create calls this once).  GHp: floats of a row of layer 0's W_in -- a multiple of 64, Hp
// being padded to 16, so a row is whole 16-byte pieces; Ep: of a row of an embedding table in front of it (0: none); n_ids: rows;
// entries: T * Bp * F; atomic: SBR_FLAG_ATOMIC_SCATTER; scat_range, tail_scatter_lds: the switches; tail_chunks: as planned
// (plan_tail; < 2: .tail is not read); units: workgroups of the LDS-row form; part_slots: rows of the partial-row slab (0: none).
// Two directions (D = 2) sort twice, the ids and the reversed ids, and each takes form 0 with its own keys: forms 1 and 2 have ONE
// partial-row slab, and the overlapped tail is never planned for them.
ScatPlan sbr_scat_plan(int GHp, int Ep, int n_ids, int entries, int D, bool atomic, int scat_range, int tail_scatter_lds,
                       int tail_chunks, int units, int part_slots) {
    ScatPlan p;      // (.plain = SCAT_REDUCE: narrow or very wide rows, two directions, the rows of an embedding table)
    const int R4 = GHp / 4;
    p.reduce = sbr_scat_reduce_recipe(Ep ? Ep : GHp);
    p.wide_rows = part_slots > 0 && sbr_scatter_wide_rows(Ep, GHp);
    const bool one_slab = p.wide_rows && D == 1;
    if (!Ep && atomic) p.plain = SCAT_ATOMIC;
    else if (scat_range == 1 && one_slab && GHp <= 1024) { p.plain = SCAT_RANGE; p.range_nv = (R4 + 255) / 256; }
    else if (scat_range == 2 && one_slab && GHp <= 2048 && part_slots >= sbr_scatter_wide_slots((size_t)entries)) {
        p.plain = SCAT_WIDE; p.wide_nvw = R4 <= 128 ? 2 : R4 <= 256 ? 4 : 8; p.wide_nvb = R4 <= 256 ? 1 : 2;
    }
    // the tail's LDS rows: ids of an average unit = 16, + the ids the cost floor admits; they must fit 120 KB, in rows up to 512 floats
    const int floor_cost = std::max(1, (entries + units * 16 - 1) / (units * 16));
    const int rows_lds = (int)((((long)entries + (long)n_ids * floor_cost + units - 1) / units) / floor_cost) + 3;
    if (tail_scatter_lds && R4 <= 128 && tail_chunks >= 1 && tail_chunks <= SBR_TCHUNKS_MAX && (size_t)rows_lds * GHp * sizeof(float) <= 120 * 1024) {
        p.tail = SCAT_LDS; p.lds_nv = R4 <= 64 ? 1 : 2; p.floor_cost = floor_cost; p.rows_lds = rows_lds;
    } else p.poll_nv = R4 <= 64 ? 1 : R4 <= 128 ? 2 : R4 <= 256 ? 4 : 0;      // (0: rows beyond 1024 floats, no kernel -- the tail is planned for 128 units only)
    return p;
}
