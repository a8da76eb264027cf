// sbr_rank_candidates / sbr_sessions_rank_candidates: ranking inside a candidate list the caller brings, one list per row
// (include/sbr_rnn.h; host code: sbr_rank_api.hip).  A candidate list is a member list that differs from row to row, so
// everything behind the scores is sbr_cluster_rank's: the exclusion by binary search in the ascending list (ExclCluster with the
// identity as "cluster" of a row), select and sort of sbr_rank.hip on the compact matrix cs [rows][lmax], crk_translate_kernel.  A
// list shared by every row is one cluster of all rows: crk_score_kernel itself scores it (cand_shared_work fills its tile table).
//
// cand_score_kernel, the scores of rows that do NOT share their list.  crk_score_kernel's tile is 16 rows x 64 shared members; here
// an MFMA takes the tile's 16 rows as operand A and, as column n of operand B, candidate p of ROW n, and keeps the diagonal D[n][n]:
// one chain of v_mfma_f32_16x16x4_f32 over K yields place p of 16 rows (15/16 of the pipe's results are dropped; by the counts --
// 2 K flops against a gather of 4 K bytes of W_out^T per candidate -- the gather bounds the kernel, not the pipe; measured so far
// are whole calls only).
//
// Accumulation order.  The argument at the top of sbr_cluster_rank.hip holds unchanged: an output element of the instruction depends
// on its own row of A and its own column of B only.  The chain runs over ascending k-blocks of 4, lane group q holding k = 4m + q,
// operand A the user representation and operand B the item's row of W_out^T, K padded with zeros to a multiple of 16; the store adds
// + 0.0f and then the bias in an f32 add of its own.  So D[n][n] is the very float sbr_rank ranks for (row n, candidate p of row n).
#include "sbr_common.h"
#include <math.h>
#include <algorithm>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kTileRows = 16;                 // rows of a tile = the M and the N of v_mfma_f32_16x16x4_f32
constexpr int kWavePlaces = 4;                // places of a wave: four independent gathers in flight per thread
constexpr int kPlaces = 4 * kWavePlaces;      // places of a workgroup of 4 waves
constexpr int kPairs = kTileRows * kPlaces;   // (place, row) pairs of a workgroup = columns of its B tile in LDS
constexpr int kBK = 16;                       // k-block staged in LDS per step (gemm_f32_mfma's BK)
constexpr int kLdB = kPairs + 4;              // LDS row strides (floats): + 4 keeps 16-byte alignment and breaks the bank period
constexpr int kLdA = kTileRows + 4;

// grid (chunks of kPlaces places, tiles of 16 consecutive rows): wave w scores places [p0 + 4 w, + 4) of the tile's rows.
// Column c = pl * 16 + j of the B tile is candidate p0 + pl of row r0 + j.
__global__ void __launch_bounds__(256) cand_score_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ W, const float* __restrict__ bout,
                                                         int K, const int* __restrict__ mem, const int* __restrict__ moff, int rows, int lmax,
                                                         float* __restrict__ cs) {
    __shared__ __attribute__((aligned(16))) float As[kBK * kLdA];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * kLdB];
    __shared__ int s_base[kTileRows], s_len[kTileRows];
    __shared__ int s_item[kPairs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.y * kTileRows, nr = min(kTileRows, rows - r0);
    const int p0 = blockIdx.x * kPlaces;
    if (tid < kTileRows) {
        const bool live = tid < nr;
        s_base[tid] = live ? moff[r0 + tid] : 0;
        s_len[tid] = live ? moff[r0 + tid + 1] - moff[r0 + tid] : 0;
    }
    __syncthreads();
    int longest = 0;
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) longest = max(longest, s_len[r]);
    {   // the item of every (place, row) pair, -1 behind the row's list
        const int pl = tid >> 4, r = tid & 15, p = p0 + pl;
        s_item[tid] = p < s_len[r] ? mem[s_base[r] + p] : -1;
    }
    __syncthreads();
    if (p0 >= longest) {                              // behind every list of the tile: -inf, never ranked
        const int pl = tid >> 4, r = tid & 15;
        if (r < nr && p0 + pl < lmax) cs[(size_t)(r0 + r) * lmax + p0 + pl] = -INFINITY;
        return;
    }
    // a thread stages four consecutive k of four candidate rows (16-byte loads of the item-major W_out^T), the first wave also of one user row
    const int ld_c = tid >> 2, ld_k = (tid & 3) << 2;
    const float* wrow[kWavePlaces];
#pragma unroll
    for (int i = 0; i < kWavePlaces; ++i) {
        const int item = s_item[ld_c + 64 * i];
        wrow[i] = item >= 0 ? W + (size_t)item * K : nullptr;
    }
    const float* hrow = (tid < 4 * kTileRows && ld_c < nr) ? h + (size_t)(r0 + ld_c) * ldh : nullptr;
    f32x4 ra = {0, 0, 0, 0}, rb[kWavePlaces];
    auto load_tile = [&](int k0) {
        const bool in = k0 + ld_k < K;                // K is a multiple of 4: a quad is inside or outside
#pragma unroll
        for (int i = 0; i < kWavePlaces; ++i) rb[i] = (wrow[i] && in) ? *(const f32x4*)(wrow[i] + k0 + ld_k) : f32x4{0, 0, 0, 0};
        ra = (hrow && in) ? *(const f32x4*)(hrow + k0 + ld_k) : f32x4{0, 0, 0, 0};
    };
    f32x4 acc[kWavePlaces];
#pragma unroll
    for (int i = 0; i < kWavePlaces; ++i) acc[i] = f32x4{0, 0, 0, 0};
    load_tile(0);
    for (int k0 = 0; k0 < K; k0 += kBK) {
        __syncthreads();                              // the previous block's MFMA reads are done
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int i = 0; i < kWavePlaces; ++i) Bs[(ld_k + e) * kLdB + ld_c + 64 * i] = rb[i][e];
            if (tid < 4 * kTileRows) As[(ld_k + e) * kLdA + ld_c] = ra[e];
        }
        __syncthreads();
        if (k0 + kBK < K) load_tile(k0 + kBK);
#pragma unroll
        for (int ks = 0; ks < kBK / 4; ++ks) {
            const float af = As[(ks * 4 + q) * kLdA + j];
#pragma unroll
            for (int i = 0; i < kWavePlaces; ++i) {
                const float bf = Bs[(ks * 4 + q) * kLdB + (wave * kWavePlaces + i) * 16 + j];
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, acc[i], 0, 0, 0);
            }
        }
    }
    asm volatile("s_nop 15");                         // MFMA D -> VALU read hazard across the loop exit (see sbr_rec.hip)
    // lane (j, q) holds D[4 q + r][j], r = 0 .. 3: the diagonal element of column j sits in lane group q = j / 4 at r = j % 4
    if ((j >> 2) == q && j < nr) {
        const int r = j & 3;
#pragma unroll
        for (int i = 0; i < kWavePlaces; ++i) {
            const int pl = wave * kWavePlaces + i, p = p0 + pl;
            if (p >= lmax) continue;
            const int item = s_item[pl * 16 + j];
            const float d = r == 0 ? acc[i][0] : r == 1 ? acc[i][1] : r == 2 ? acc[i][2] : acc[i][3];
            // (+ 0.0f: gemm_f32_mfma's store without a bias; then softmax_rows_kernel's add)
            cs[(size_t)(r0 + j) * lmax + p] = item >= 0 ? (d + 0.0f) + bout[item] : -INFINITY;
        }
    }
}

}  // namespace

hipError_t launch_cand_score(hipStream_t s, const float* h, int ldh, const float* WoutT, const float* bout, int K, const int* cand_ids,
                             const int* cand_off, int rows, int lmax, float* cs) {
    if (rows <= 0) return hipSuccess;
    if (K % 4 || ldh % 4 || lmax < 1) return hipErrorInvalidValue;
    cand_score_kernel<<<dim3((unsigned)((lmax + kPlaces - 1) / kPlaces), (unsigned)((rows + kTileRows - 1) / kTileRows)), 256, 0, s>>>(
        h, ldh, WoutT, bout, K, cand_ids, cand_off, rows, lmax, cs);
    return hipGetLastError();
}

// launch_crk_group's words for ONE cluster that every row selects, filled on the host: the rows in their own order, tiles of 16
// consecutive rows (the layout launch_crk_score reads: counts [1], offsets [2], order [rows], tiles [3][max_tiles], n_tiles [1])
void cand_shared_work(int rows, int* work) {
    const int mt = sbr_crk_max_tiles(rows, 1);
    int* cnt = work; int* off = cnt + 1; int* order = off + 2; int* tiles = order + rows; int* n_tiles = tiles + 3 * (size_t)mt;
    cnt[0] = rows; off[0] = 0; off[1] = rows;
    for (int r = 0; r < rows; ++r) order[r] = r;
    int nt = 0;
    for (int f = 0; f < rows; f += kTileRows, ++nt) { tiles[nt] = 0; tiles[mt + nt] = f; tiles[2 * mt + nt] = std::min(kTileRows, rows - f); }
    for (int t = nt; t < mt; ++t) tiles[t] = tiles[mt + t] = tiles[2 * mt + t] = 0;
    *n_tiles = nt;
}
