// sbr_cluster_lists / sbr_cluster_rank: ranking inside each row's item cluster (include/sbr_rnn.h; the batched, device form of
// RNNCluster.predict_function, rnn_cluster.py:302-325, over the hard clusters of prepare_tests, :440-466).
//
//   lists     once per version of R: crk_count_kernel (per block of 256 consecutive ids, members per cluster), crk_prefix_kernel
//             (exclusive offsets of the blocks inside every list, list sizes), crk_offsets_kernel (first entry of every list),
//             crk_fill_kernel (ordered compaction: a block's members land behind those of the blocks before it, a wave's behind the
//             waves before it, a lane's behind the lower lanes -- every list ascending in id, no atomics)
//   per call  crk_group_kernel (counting sort of the rows by cluster, table of 16-row tiles), then either
//             crk_score_kernel  (form 1) the scores of the members only, into a compact matrix cs [rows][Lmax], or
//             crk_gather_kernel (form 2) the same places picked out of the full score matrix,
//             the exclusion (sbr_rank.hip's exclude_kernel on ExclCluster rows: binary search of every excluded id in the row's
//             ascending list), the select and sort of sbr_rank.hip on cs (they return PLACES; place order inside a list is id order, so their tie rule carries over),
//             crk_translate_kernel (place -> item id).
//
// Accumulation order of form 1.  full_scores runs gemm_f32_mfma (sbr_gemm.hip) without split-K: for an output element one chain of
// v_mfma_f32_16x16x4_f32 over ascending k-blocks of 4, lane group q of the instruction holding k = 4m + q, operand A the user
// representation and operand B the item's row of W_out^T, K padded with zeros to a multiple of 16; the store adds +0.0f and
// softmax_rows_kernel then adds the bias as an f32 add of its own.  crk_score_kernel issues the same instruction on the same operand
// roles in the same k order and ends in the same two adds, so a score here is the very float sbr_rank ranks: an output element of
// the instruction depends on its own row of A and column of B only, not on which rows or items share the tile.
#include "sbr_common.h"
#include <math.h>
#include <algorithm>
#include <new>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CRK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { sbr_set_error("%s: %s", #x, hipGetErrorString(e_)); return SBR_EHIP; } } while (0)
#define CRK_ARG(c, ...) do { if (!(c)) { sbr_set_error(__VA_ARGS__); return SBR_EINVAL; } } while (0)

namespace {

constexpr int kMaxClusters = 8192;    // the per-cluster tables of a workgroup sit in LDS (4 waves x C counters: 128 KB at the limit)
constexpr int kBlockIds = 256;        // consecutive ids of a workgroup of the list build
constexpr int kTileRows = 16;         // rows of a tile = the M of v_mfma_f32_16x16x4_f32
constexpr int kChunk = 64;            // members of a workgroup of the scoring kernel: a cluster of a few hundred members spreads over several CUs
constexpr int kBK = 16;               // k-block staged in LDS per step (gemm_f32_mfma's BK)
constexpr int kLdB = kChunk + 4;      // LDS row strides (floats): + 4 keeps 16-byte alignment and breaks the bank period
constexpr int kLdA = kTileRows + 4;

// the fallback cluster of an item none of whose memberships is positive -- the reference's literal scan (rnn_cluster.py:447-458:
// it starts from cluster 0's value and only a strictly larger one replaces it; NaN compares false) -- or -1 for an item with a
// positive membership
__device__ __forceinline__ int crk_fallback(const float* __restrict__ r, int C) {
    int best = 0;
    float bv = r[0];
    bool pos = bv > 0.0f;
    for (int j = 1; j < C; ++j) {
        const float v = r[j];
        if (v > bv) { bv = v; best = j; }
        pos |= v > 0.0f;
    }
    return pos ? -1 : best;
}

// wcnt[w][c] = members of cluster c among the 64 ids of wave w (LDS, [4][C])
__device__ __forceinline__ void crk_wave_counts(const float* __restrict__ R, int N, int C, int i, int fb, unsigned* wcnt) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = 0; c < C; ++c) {
        const bool m = i < N && (R[(size_t)i * C + c] > 0.0f || fb == c);
        const unsigned long long b = __ballot(m);
        if (lane == 0) wcnt[w * C + c] = (unsigned)__popcll(b);
    }
}

__global__ void __launch_bounds__(kBlockIds) crk_count_kernel(const float* __restrict__ R, int N, int C, int nb, int* __restrict__ bcnt) {
    extern __shared__ unsigned wcnt[];
    const int i = blockIdx.x * kBlockIds + threadIdx.x;
    const int fb = i < N ? crk_fallback(R + (size_t)i * C, C) : -2;
    crk_wave_counts(R, N, C, i, fb, wcnt);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kBlockIds)
        bcnt[(size_t)c * nb + blockIdx.x] = (int)(wcnt[c] + wcnt[C + c] + wcnt[2 * C + c] + wcnt[3 * C + c]);
}

// one wave per cluster: bcnt[c][b] becomes the members of cluster c in the blocks before b; size[c] their total
__global__ void __launch_bounds__(64) crk_prefix_kernel(int* __restrict__ bcnt, int nb, int* __restrict__ size) {
    const int c = blockIdx.x, lane = threadIdx.x;
    int* row = bcnt + (size_t)c * nb;
    int run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {             // wave-uniform trip count
        const int b = b0 + lane;
        const int v = b < nb ? row[b] : 0;
        int s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o); if (lane >= o) s += t; }
        if (b < nb) row[b] = run + s - v;
        run += __shfl(s, 63);
    }
    if (lane == 0) size[c] = run;
}

__global__ void crk_offsets_kernel(const int* __restrict__ size, int C, int* __restrict__ off) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int run = 0;
        for (int c = 0; c < C; ++c) { off[c] = run; run += size[c]; }
        off[C] = run;
    }
}

__global__ void __launch_bounds__(kBlockIds) crk_fill_kernel(const float* __restrict__ R, int N, int C, int nb, const int* __restrict__ boff,
                                                             const int* __restrict__ off, int* __restrict__ mem, int cap) {
    extern __shared__ unsigned wcnt[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * kBlockIds + threadIdx.x;
    const int fb = i < N ? crk_fallback(R + (size_t)i * C, C) : -2;
    crk_wave_counts(R, N, C, i, fb, wcnt);
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int c = 0; c < C; ++c) {
        const bool m = i < N && (R[(size_t)i * C + c] > 0.0f || fb == c);
        const unsigned long long b = __ballot(m);
        if (m) {
            unsigned before = 0;
            for (int v = 0; v < w; ++v) before += wcnt[v * C + c];
            const int at = off[c] + boff[(size_t)c * nb + blockIdx.x] + (int)before + __popcll(b & lt);
            if (at < cap) mem[at] = i;            // (cap = off[C]: what the two passes over the same R agree on)
        }
    }
}

// one workgroup: counting sort of the rows by cluster and the tile table.  LDS: cnt [C], cur [C]
__global__ void __launch_bounds__(256) crk_group_kernel(const int* __restrict__ csel, int rows, int C, int max_tiles, int* __restrict__ cnt,
                                                        int* __restrict__ off, int* __restrict__ order, int* __restrict__ tiles,
                                                        int* __restrict__ n_tiles) {
    extern __shared__ int lds[];
    int* s_cnt = lds;
    int* s_cur = lds + C;
    for (int c = threadIdx.x; c < C; c += 256) s_cnt[c] = 0;
    __syncthreads();
    for (int r = threadIdx.x; r < rows; r += 256) {
        const int c = csel[r];
        if ((unsigned)c < (unsigned)C) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0, nt = 0;
        for (int c = 0; c < C; ++c) {
            const int g = s_cnt[c];
            s_cur[c] = run; off[c] = run; cnt[c] = g;
            for (int f = 0; f < g && nt < max_tiles; f += kTileRows, ++nt) {
                tiles[nt] = c; tiles[max_tiles + nt] = run + f; tiles[2 * max_tiles + nt] = min(kTileRows, g - f);
            }
            run += g;
        }
        off[C] = run;
        *n_tiles = nt;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < rows; r += 256) {     // (which place of its group a row takes does not reach its result)
        const int c = csel[r];
        if ((unsigned)c < (unsigned)C) order[atomicAdd(&s_cur[c], 1)] = r;
    }
}

// grid (chunks of kChunk places, tiles): wave w scores places [p0 + 16 w, + 16) for the tile's 16 rows
__global__ void __launch_bounds__(256) crk_score_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ W, const float* __restrict__ bout,
                                                        int K, const int* __restrict__ mem, const int* __restrict__ moff, const int* __restrict__ order,
                                                        const int* __restrict__ tiles, int max_tiles, const int* __restrict__ n_tiles, int lmax,
                                                        float* __restrict__ cs) {
    __shared__ __attribute__((aligned(16))) float As[kBK * kLdA];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * kLdB];
    __shared__ int s_row[kTileRows];
    __shared__ int s_item[kChunk];
    const int tile = blockIdx.y;
    if (tile >= *n_tiles) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    const int c = tiles[tile], first = tiles[max_tiles + tile], nr = tiles[2 * max_tiles + tile];
    const int base = moff[c], len = moff[c + 1] - base;
    const int p0 = blockIdx.x * kChunk;
    if (tid < kTileRows) s_row[tid] = tid < nr ? order[first + tid] : -1;
    if (tid < kChunk) s_item[tid] = p0 + tid < len ? mem[base + p0 + tid] : -1;
    __syncthreads();
    if (p0 >= len) {                                  // behind the row's list: -inf, never ranked
        for (int e = tid; e < kTileRows * kChunk; e += 256) {
            const int r = e / kChunk, n = e % kChunk;
            if (r < nr && p0 + n < lmax) cs[(size_t)s_row[r] * lmax + p0 + n] = -INFINITY;
        }
        return;
    }
    // a thread stages four consecutive k of one member row (16-byte loads of the item-major W_out^T), the first wave also of one user row
    const int ld_m = tid >> 2, ld_k = (tid & 3) << 2;
    const float* wrow = s_item[ld_m] >= 0 ? W + (size_t)s_item[ld_m] * K : nullptr;
    const float* hrow = (tid < 4 * kTileRows && s_row[ld_m] >= 0) ? h + (size_t)s_row[ld_m] * ldh : nullptr;
    f32x4 ra = {0, 0, 0, 0}, rb = {0, 0, 0, 0};
    auto load_tile = [&](int k0) {
        const bool in = k0 + ld_k < K;                // K is a multiple of 4: a quad is inside or outside
        rb = (wrow && in) ? *(const f32x4*)(wrow + k0 + ld_k) : f32x4{0, 0, 0, 0};
        ra = (hrow && in) ? *(const f32x4*)(hrow + k0 + ld_k) : f32x4{0, 0, 0, 0};
    };
    f32x4 acc = {0, 0, 0, 0};
    load_tile(0);
    for (int k0 = 0; k0 < K; k0 += kBK) {
        __syncthreads();                              // the previous block's MFMA reads are done
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Bs[(ld_k + e) * kLdB + ld_m] = rb[e];
            if (tid < 4 * kTileRows) As[(ld_k + e) * kLdA + ld_m] = ra[e];
        }
        __syncthreads();
        if (k0 + kBK < K) load_tile(k0 + kBK);
#pragma unroll
        for (int ks = 0; ks < kBK / 4; ++ks) {
            const float af = As[(ks * 4 + q) * kLdA + j];
            const float bf = Bs[(ks * 4 + q) * kLdB + wave * 16 + j];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, acc, 0, 0, 0);
        }
    }
    asm volatile("s_nop 15");                         // MFMA D -> VALU read hazard across the loop exit (see sbr_rec.hip)
    const int n = wave * 16 + j, p = p0 + n;
    if (p < lmax) {
        const int item = s_item[n];
        const float bv = item >= 0 ? bout[item] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = q * 4 + r;
            // (+ 0.0f: gemm_f32_mfma's store without a bias; then softmax_rows_kernel's add)
            if (m < nr) cs[(size_t)s_row[m] * lmax + p] = item >= 0 ? (acc[r] + 0.0f) + bv : -INFINITY;
        }
    }
}

__global__ void __launch_bounds__(256) crk_gather_kernel(const float* __restrict__ lg, int N, const int* __restrict__ csel, const int* __restrict__ mem,
                                                         const int* __restrict__ moff, int lmax, float* __restrict__ cs) {
    const int r = blockIdx.y, c = csel[r];
    const int base = moff[c], len = moff[c + 1] - base;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < lmax; p += gridDim.x * 256)
        cs[(size_t)r * lmax + p] = p < len ? lg[(size_t)r * N + mem[base + p]] : -INFINITY;
}

__global__ void __launch_bounds__(256) crk_translate_kernel(const int* __restrict__ pos, const float* __restrict__ psc, int kk, int k,
                                                            const int* __restrict__ csel, const int* __restrict__ mem, const int* __restrict__ moff,
                                                            int* __restrict__ out_ids, float* __restrict__ out_scores, int* __restrict__ size) {
    const int r = blockIdx.x, c = csel[r];
    const int base = moff[c], n = moff[c + 1] - base;
    for (int jj = threadIdx.x; jj < k; jj += 256) {
        const int p = jj < kk ? pos[(size_t)r * kk + jj] : -1;
        const bool ok = p >= 0 && p < n;
        out_ids[(size_t)r * k + jj] = ok ? mem[base + p] : -1;
        out_scores[(size_t)r * k + jj] = ok ? psc[(size_t)r * kk + jj] : -INFINITY;
    }
    if (threadIdx.x == 0 && size) size[r] = n;
}

int crk_alloc(int** p, size_t* have, size_t want, const char* what) {
    if (want <= *have && *p) return SBR_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
    const size_t bytes = std::max<size_t>(want, 1) * sizeof(int);
    if (hipMalloc((void**)p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        sbr_set_error("sbr_cluster_lists: hipMalloc(%zu) of %s failed", bytes, what);
        return SBR_ENOMEM;
    }
    *have = want;
    return SBR_OK;
}

}  // namespace

int sbr_cluster_build_lists(sbr_cluster* k) {
    if (k->lists_valid) return SBR_OK;
    const int N = k->cfg.n_items, C = k->cfg.n_clusters;
    CRK_ARG(C <= kMaxClusters, "sbr_cluster_lists: %d clusters, at most %d", C, kMaxClusters);
    const int nb = (N + kBlockIds - 1) / kBlockIds;
    int rc;
    size_t off_have = k->mem_off ? (size_t)C + 1 : 0;
    if ((rc = crk_alloc(&k->mem_off, &off_have, (size_t)C + 1, "the list offsets")) != SBR_OK) return rc;
    if ((rc = crk_alloc(&k->mem_work, &k->mem_work_n, (size_t)C * nb + C, "the per-block counts")) != SBR_OK) return rc;
    int* size_dev = k->mem_work + (size_t)C * nb;
    const size_t lds = (size_t)4 * C * sizeof(unsigned);
    SBR_DYN_LDS(crk_count_kernel, lds);
    SBR_DYN_LDS(crk_fill_kernel, lds);
    crk_count_kernel<<<nb, kBlockIds, lds, k->stream>>>(k->R, N, C, nb, k->mem_work);
    crk_prefix_kernel<<<C, 64, 0, k->stream>>>(k->mem_work, nb, size_dev);
    crk_offsets_kernel<<<1, 64, 0, k->stream>>>(size_dev, C, k->mem_off);
    CRK_HIP(hipGetLastError());
    k->mem_sizes.assign((size_t)C, 0);
    CRK_HIP(hipMemcpyAsync(k->mem_sizes.data(), size_dev, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, k->stream));
    CRK_HIP(hipStreamSynchronize(k->stream));        // once per version of R: a rank call sizes everything from the host copy
    size_t total = 0;
    int longest = 0;
    for (int c = 0; c < C; ++c) { total += (size_t)k->mem_sizes[c]; longest = std::max(longest, k->mem_sizes[c]); }
    if ((rc = crk_alloc(&k->mem_ids, &k->mem_cap, total, "the member lists")) != SBR_OK) return rc;
    crk_fill_kernel<<<nb, kBlockIds, lds, k->stream>>>(k->R, N, C, nb, k->mem_work, k->mem_off, k->mem_ids, (int)total);
    CRK_HIP(hipGetLastError());
    k->lmax = std::max(4, (longest + 3) / 4 * 4);
    k->lists_valid = 1;
    return SBR_OK;
}

extern "C" int sbr_cluster_lists(sbr_cluster* k, int32_t* sizes_host, int32_t* members_host) {
    CRK_ARG(k && sizes_host, "null argument");
    const int rc = sbr_cluster_build_lists(k);
    if (rc != SBR_OK) return rc;
    size_t total = 0;
    for (int c = 0; c < k->cfg.n_clusters; ++c) { sizes_host[c] = k->mem_sizes[c]; total += (size_t)k->mem_sizes[c]; }
    if (members_host && total) {
        CRK_HIP(hipMemcpyAsync(members_host, k->mem_ids, total * sizeof(int), hipMemcpyDeviceToHost, k->stream));
        CRK_HIP(hipStreamSynchronize(k->stream));
    }
    return SBR_OK;
}

hipError_t launch_crk_group(hipStream_t s, const int* csel, int rows, int C, int* work) {
    if (rows <= 0) return hipSuccess;
    const int mt = sbr_crk_max_tiles(rows, C);
    int* cnt = work; int* off = cnt + C; int* order = off + C + 1; int* tiles = order + rows; int* n_tiles = tiles + 3 * (size_t)mt;
    const size_t lds = (size_t)2 * C * sizeof(int);
    SBR_DYN_LDS(crk_group_kernel, lds);
    crk_group_kernel<<<1, 256, lds, s>>>(csel, rows, C, mt, cnt, off, order, tiles, n_tiles);
    return hipGetLastError();
}

hipError_t launch_crk_score(hipStream_t s, const float* h, int ldh, const float* WoutT, const float* bout, int K, const int* mem_ids,
                            const int* mem_off, const int* work, int rows, int C, int lmax, float* cs) {
    if (rows <= 0) return hipSuccess;
    if (K % 4 || ldh % 4 || lmax < 1) return hipErrorInvalidValue;
    const int mt = sbr_crk_max_tiles(rows, C);
    const int* order = work + C + (C + 1); const int* tiles = order + rows; const int* n_tiles = tiles + 3 * (size_t)mt;
    crk_score_kernel<<<dim3((unsigned)((lmax + kChunk - 1) / kChunk), (unsigned)mt), 256, 0, s>>>(h, ldh, WoutT, bout, K, mem_ids, mem_off, order, tiles,
                                                                                                 mt, n_tiles, lmax, cs);
    return hipGetLastError();
}

hipError_t launch_crk_gather(hipStream_t s, const float* logits, int N, const int* csel, const int* mem_ids, const int* mem_off,
                             int rows, int lmax, float* cs) {
    if (rows <= 0) return hipSuccess;
    crk_gather_kernel<<<dim3((unsigned)std::min(64, (lmax + 255) / 256), (unsigned)rows), 256, 0, s>>>(logits, N, csel, mem_ids, mem_off, lmax, cs);
    return hipGetLastError();
}

hipError_t launch_crk_translate(hipStream_t s, const int* pos, const float* psc, int kk, int k, const int* csel, const int* mem_ids,
                                const int* mem_off, int rows, int* out_ids, float* out_scores, int* size) {
    if (rows <= 0) return hipSuccess;
    crk_translate_kernel<<<rows, 256, 0, s>>>(pos, psc, kk, k, csel, mem_ids, mem_off, out_ids, out_scores, size);
    return hipGetLastError();
}
