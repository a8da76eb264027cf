// K13 optimizers, the dense step kernels: lasagne.updates.{adagrad,adadelta,rmsprop,nesterov_momentum,adam} [3P]
// (update_manager.py:24-82) applied to flat ranges of the parameter section.  Every kernel here holds an element's gradient,
// parameter and state in registers and calls upd_step (sbr_upd.h); the row-sparse steps are in sbr_sparse.hip.
#include "sbr_common.h"
#include "sbr_device.h"

__global__ void update_kernel(SbrUpdRule st, float* __restrict__ p, float* __restrict__ g, float* __restrict__ s0,
                              float* __restrict__ s1, size_t n, size_t gap_at, size_t gap_len) {
    // n elements of [0, gap_at) u [gap_at + gap_len, ...): two parameter ranges in one launch
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        const size_t i = k < gap_at ? k : k + gap_len;
        const float gi = g[i];
        g[i] = 0.0f;                                      // the gradient section is clean for the next step (no memset)
        float pi = p[i], ai = s0[i], bi = s1 ? s1[i] : 0.0f;
        upd_step(st, gi, pi, ai, bi);
        p[i] = pi; s0[i] = ai;
        if (s1) s1[i] = bi;
    }
}

hipError_t launch_update(hipStream_t s, const SbrUpdRule& st, float* p, float* g, float* s0, float* s1, size_t n, size_t gap_at,
                         size_t gap_len) {
    if (n == 0) return hipSuccess;
    const int grid = (int)min((size_t)256 * 16, (n + 255) / 256);
    update_kernel<<<grid, 256, 0, s>>>(st, p, g, s0, s1, n, gap_at, gap_len);
    return hipGetLastError();
}

// The optimizer step of a parameter block whose gradient still lies in split-K slabs (dW_hid of the overlapped step tail): the
// slab reduction of gemm_splitk_reduce_v4 -- same grouping, same summation order, so the same gradient bits -- with the step
// applied by the thread that holds the finished sum.  One launch and one pass over the block less at the end of the step; the
// gradient array itself is not written (it stays as the last update left it: zero).
__global__ void __launch_bounds__(256) update_from_slabs_kernel(SbrUpdRule st, const f32x4* __restrict__ ws, int nsplit, size_t n,
                                                                float* __restrict__ p, float* __restrict__ s0, float* __restrict__ s1) {
    __shared__ f32x4 red[16][16];
    const size_t n4 = n / 4;
    const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const size_t i4 = (size_t)blockIdx.x * 16 + j;
    f32x4 a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0;
    if (i4 < n4) {
        int z = grp;
        for (; z + 48 < nsplit; z += 64) {
            a0 += ws[(size_t)z * n4 + i4]; a1 += ws[(size_t)(z + 16) * n4 + i4];
            a2 += ws[(size_t)(z + 32) * n4 + i4]; a3 += ws[(size_t)(z + 48) * n4 + i4];
        }
        for (; z < nsplit; z += 16) a0 += ws[(size_t)z * n4 + i4];
    }
    red[grp][j] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int jj = threadIdx.x >> 2, e = threadIdx.x & 3;             // one element per thread
    const size_t i = ((size_t)blockIdx.x * 16 + jj) * 4 + e;
    if (i >= n) return;
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g][jj][e];
    float pi = p[i], ai = s0[i], bi = s1 ? s1[i] : 0.0f;
    upd_step(st, t, pi, ai, bi);
    p[i] = pi; s0[i] = ai;
    if (s1) s1[i] = bi;
}

hipError_t launch_update_from_slabs(hipStream_t s, const SbrUpdRule& st, const float* ws, int nslabs, float* p, float* s0, float* s1,
                                    size_t n) {
    if (n == 0) return hipSuccess;
    if ((n & 3) || ((uintptr_t)ws & 15)) return hipErrorInvalidValue;
    update_from_slabs_kernel<<<(unsigned)((n / 4 + 15) / 16), 256, 0, s>>>(st, (const f32x4*)ws, nslabs, n, p, s0, s1);
    return hipGetLastError();
}

// The dense pass over an item-indexed block, aware of which rows the batch touched (offs = the scatter's segment offsets): an
// untouched row's gradient is zero and stays zero, so its step reads and writes p, s0, s1 only (6 passes instead of 8: C4 touches 40 %
// of its 26 744 rows per batch); a touched row's gradient is read and cleared as update_kernel does.  One streaming launch, 16
// bytes per lane.
__global__ void __launch_bounds__(256) update_rows_aware_kernel(SbrUpdRule st, f32x4* __restrict__ p, f32x4* __restrict__ g,
                                                                f32x4* __restrict__ s0, f32x4* __restrict__ s1, int n_rows, int R4,
                                                                const int* __restrict__ offs) {
    const size_t n4 = (size_t)n_rows * R4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / (unsigned)R4);
        const bool touched = offs[r + 1] > offs[r];
        f32x4 gv = {0, 0, 0, 0};
        if (touched) { gv = g[i]; g[i] = f32x4{0, 0, 0, 0}; }
        f32x4 pv = p[i], av = s0[i], bv = s1 ? s1[i] : f32x4{0, 0, 0, 0};
        upd_step4(st, gv, pv, av, bv);
        p[i] = pv; s0[i] = av;
        if (s1) s1[i] = bv;
    }
}
hipError_t launch_update_rows_aware(hipStream_t s, const SbrUpdRule& st, float* p, float* g, float* s0, float* s1, int n_rows,
                                    int row_floats, const int* offs) {
    if (n_rows <= 0) return hipSuccess;
    if ((row_floats & 3) || !offs) return hipErrorInvalidValue;
    const size_t n4 = (size_t)n_rows * (row_floats / 4);
    const int grid = (int)min((size_t)256 * 16, (n4 + 255) / 256);
    update_rows_aware_kernel<<<grid, 256, 0, s>>>(st, (f32x4*)p, (f32x4*)g, (f32x4*)s0, (f32x4*)s1, n_rows, row_floats / 4, offs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The output layer's gradient AND its optimizer step in one launch (round 5; single-call steps of the dense heads, no bias
// regulariser): dW_out^T[n][k] = sum_rows dlogits[row][n] h[row][k], db[n] = sum_rows dlogits[row][n], cost = sum_rows rowcost
// (rnn_one_hot.py:65-77 backward + update_manager.py:24-82).  Before: sum_cost, two column-sum kernels, the dW_out GEMM (+ its
// split-K reduction) and update_kernel -- five to six launches, 50 - 60 us with their gaps on the side stream, IN FRONT of the
// polling weight-gradient GEMM of the overlapped tail, which therefore started 68 us into a 138 us BPTT chain and ended 39 us
// behind it (profiles/round4_z_c2_timeline.txt).  Here a workgroup owns 16 items: its four waves split the batch rows, every
// wave accumulates D[k][item] over its rows on v_mfma_f32_16x16x4_f32 (k slot q = row r0 + q; operands straight from L2: 64
// contiguous bytes per 16 lanes), the partial sums meet in LDS, and the thread that holds four consecutive k of an item steps
// W_out^T[item][k .. k + 3] (upd_step4); the gradient arrays are never written (they stay zero).
// ---------------------------------------------------------------------------------------
template <int HP>
__global__ void __launch_bounds__(256) out_grad_step_kernel(const float* __restrict__ dlog, const float* __restrict__ h,
                                                            const float* __restrict__ rowcost, float* __restrict__ cost, SbrUpdRule st,
                                                            float* __restrict__ Wp, float* __restrict__ Ws0, float* __restrict__ Ws1,
                                                            float* __restrict__ bp, float* __restrict__ bs0, float* __restrict__ bs1,
                                                            int R, int N, int Nl) {
    constexpr int KG = HP / 16;
    __shared__ __attribute__((aligned(16))) f32x4 part[4][KG][64];
    __shared__ float dbp[4][16];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const bool col_in = n0 + j < N;
    const int rpw = ((R + 3) / 4 + 3) / 4 * 4;                       // rows per wave, a multiple of 4
    const int r_lo = wave * rpw, r_hi = min(R, r_lo + rpw);
    f32x4 acc[KG];
#pragma unroll
    for (int kt = 0; kt < KG; ++kt) acc[kt] = f32x4{0, 0, 0, 0};
    float dbv = 0.0f;
    for (int r0 = r_lo; r0 < r_hi; r0 += 16) {                      // four row groups per round: their 4 + 4 KG loads in flight together
        float d[4], hv[4][KG];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = r0 + 4 * u + q;
            const bool in = row < r_hi;
            d[u] = (in && col_in) ? dlog[(size_t)row * Nl + n0 + j] : 0.0f;
            const float* hr = h + (size_t)(in ? row : r_lo) * HP + j;
#pragma unroll
            for (int kt = 0; kt < KG; ++kt) hv[u][kt] = in ? hr[16 * kt] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            dbv += d[u];
#pragma unroll
            for (int kt = 0; kt < KG; ++kt) acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[u][kt], d[u], acc[kt], 0, 0, 0);
        }
    }
    asm volatile("s_nop 15");                                        // MFMA D -> VALU read across the loop exit
#pragma unroll
    for (int kt = 0; kt < KG; ++kt) part[wave][kt][lane] = acc[kt];
    dbv += __shfl_xor(dbv, 16); dbv += __shfl_xor(dbv, 32);
    if (q == 0) dbp[wave][j] = dbv;
    if (blockIdx.x == 0) {                                           // the batch cost: fixed order
        float c = 0.0f;
        for (int r = tid; r < R; r += 256) c += rowcost[r];
        c = block_sum(c, red);
        if (tid == 0) *cost = c;
    }
    __syncthreads();
    for (int i = tid; i < KG * 64; i += 256) {
        const int kt = i >> 6, ln = i & 63, item = n0 + (ln & 15), k = 16 * kt + 4 * (ln >> 4);
        if (item >= N) continue;
        const f32x4 g = (part[0][kt][ln] + part[1][kt][ln]) + (part[2][kt][ln] + part[3][kt][ln]);
        const size_t o = (size_t)item * HP + k;
        f32x4 pv = *(const f32x4*)(Wp + o), av = *(const f32x4*)(Ws0 + o), bv = Ws1 ? *(const f32x4*)(Ws1 + o) : f32x4{0, 0, 0, 0};
        upd_step4(st, g, pv, av, bv);
        *(f32x4*)(Wp + o) = pv; *(f32x4*)(Ws0 + o) = av;
        if (Ws1) *(f32x4*)(Ws1 + o) = bv;
    }
    if (tid < 16 && n0 + tid < N) {
        const float g = (dbp[0][tid] + dbp[1][tid]) + (dbp[2][tid] + dbp[3][tid]);
        float pe = bp[n0 + tid], ae = bs0[n0 + tid], be = bs1 ? bs1[n0 + tid] : 0.0f;
        upd_step(st, g, pe, ae, be);
        bp[n0 + tid] = pe; bs0[n0 + tid] = ae;
        if (bs1) bs1[n0 + tid] = be;
    }
}

// W: W_out^T [N][Hp] with its state arrays (s1 NULL: one state array), b: b_out [N] likewise; false: shape not served
bool launch_out_grad_step(hipStream_t s, const SbrUpdRule& st, const float* dlogits, const float* h_last, const float* rowcost,
                          float* cost, float* W, float* Ws0, float* Ws1, float* b, float* bs0, float* bs1, int R, int N, int Nl, int Hp,
                          hipError_t* err) {
    if (!(Hp == 32 || Hp == 64 || Hp == 128) || R < 1 || N < 1) return false;
    const int grid = (N + 15) / 16;
    if (Hp == 128) out_grad_step_kernel<128><<<grid, 256, 0, s>>>(dlogits, h_last, rowcost, cost, st, W, Ws0, Ws1, b, bs0, bs1, R, N, Nl);
    else if (Hp == 64) out_grad_step_kernel<64><<<grid, 256, 0, s>>>(dlogits, h_last, rowcost, cost, st, W, Ws0, Ws1, b, bs0, bs1, R, N, Nl);
    else out_grad_step_kernel<32><<<grid, 256, 0, s>>>(dlogits, h_last, rowcost, cost, st, W, Ws0, Ws1, b, bs0, bs1, R, N, Nl);
    *err = hipGetLastError();
    return true;
}
