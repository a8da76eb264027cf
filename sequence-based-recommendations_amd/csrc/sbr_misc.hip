// HBM-bound and small kernels of the hot path (gfx950, wave64): embedding-bag gather (K1; its
// scatter-add gradient, K6: sbr_scatter.hip), softmax / cross-entropy (K8), sampled heads (K10-K12),
// test-path exclusion + top-k (K14).  (The optimizers, K13: sbr_upd.h, sbr_update.hip.)
#include "sbr_common.h"
#include "sbr_rec_p.h"
#include "sbr_device.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// block-wide reductions (256 threads = 4 waves): sbr_device.h

// ---------------------------------------------------------------------------------------
// K1 embedding-bag gather: xt[t][b][:] = sum_f W_in[X[b][t][f]][:] + bias
// (sparse_lstm.py:368 / :755 / :1111).  One 16-byte piece per thread: a row of G*Hp floats is
// read by G*Hp/4 consecutive lanes (coalesced 16 B/lane), written the same way.
// ---------------------------------------------------------------------------------------
__global__ void gather_xt_kernel(const f32x4* __restrict__ Win, const f32x4* __restrict__ bias,
                                 const int* __restrict__ X, f32x4* __restrict__ xt, int T, int Bp, int F, int R4) {
    const size_t total = (size_t)T * Bp * R4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int f4 = (int)(i % R4);
        const size_t pos = i / R4;
        const int b = (int)(pos % Bp), t = (int)(pos / Bp);
        f32x4 v = bias[f4];
        const int* ids = X + ((size_t)b * T + t) * F;
        for (int f = 0; f < F; ++f) v += Win[(size_t)ids[f] * R4 + f4];
        xt[i] = v;
    }
}

__global__ void gather_concat_kernel(const f32x4* __restrict__ W, const int* __restrict__ X, f32x4* __restrict__ out, int T,
                                     int Bp, int F, int E4) {
    const size_t total = (size_t)T * Bp * F * E4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e4 = (int)(i % E4);
        const size_t pf = i / E4;                      // (t*Bp + b)*F + f
        const int f = (int)(pf % F);
        const size_t pos = pf / F;
        const int b = (int)(pos % Bp), t = (int)(pos / Bp);
        out[i] = W[(size_t)X[((size_t)b * T + t) * F + f] * E4 + e4];
    }
}
hipError_t launch_gather_concat(hipStream_t s, const float* Wemb, const int* X, float* out, int T, int Bp, int F, int Ep) {
    const size_t total = (size_t)T * Bp * F * (Ep / 4);
    const int grid = (int)min((size_t)256 * 16, (total + 255) / 256);
    gather_concat_kernel<<<grid, 256, 0, s>>>((const f32x4*)Wemb, X, (f32x4*)out, T, Bp, F, Ep / 4);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// --r_bi helpers.  The backwards layer of a level (Lasagne go_backwards=True over the left-aligned, masked sequence:
// the padded steps come first and copy hid_init, then the valid steps in reverse) is run as an ordinary forward scan
// over the row's valid steps REVERSED IN PLACE: rev(t) = len-1-t for t < len, t otherwise.  State after scan step s of
// the reversed row = the backwards layer's output at time len-1-s; its final state = the output at time 0, which is what
// only_return_final takes (sparse_lstm.py:485-486).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int rev_t(int t, int len) { return t < len ? len - 1 - t : t; }

__global__ void rev_rows_int_kernel(const int* __restrict__ X, const int* __restrict__ len, int* __restrict__ Xr, int T, int Bp, int F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Bp * T * F) return;
    const int f = i % F, t = (i / F) % T, b = i / (F * T);
    Xr[i] = X[((size_t)b * T + rev_t(t, len[b])) * F + f];
}
hipError_t launch_rev_rows_int(hipStream_t s, const int* X, const int* len, int* Xr, int T, int Bp, int F) {
    const int n = Bp * T * F;
    rev_rows_int_kernel<<<(n + 255) / 256, 256, 0, s>>>(X, len, Xr, T, Bp, F);
    return hipGetLastError();
}

__global__ void rev_rows_kernel(const f32x4* __restrict__ src, const int* __restrict__ len, f32x4* __restrict__ dst, int T, int Bp, int W4) {
    const size_t total = (size_t)T * Bp * W4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(i % W4);
        const size_t pos = i / W4;
        const int b = (int)(pos % Bp), t = (int)(pos / Bp);
        dst[i] = src[((size_t)rev_t(t, len[b]) * Bp + b) * W4 + w];
    }
}
hipError_t launch_rev_rows(hipStream_t s, const float* src, const int* len, float* dst, int T, int Bp, int W) {
    const size_t total = (size_t)T * Bp * (W / 4);
    rev_rows_kernel<<<(int)min((size_t)4096, (total + 255) / 256), 256, 0, s>>>((const f32x4*)src, len, (f32x4*)dst, T, Bp, W / 4);
    return hipGetLastError();
}

__global__ void cat_outputs_kernel(const f32x4* __restrict__ hf, const f32x4* __restrict__ hb, const int* __restrict__ len,
                                   f32x4* __restrict__ cat, int T, int Bp, int H4) {
    const size_t total = (size_t)T * Bp * 2 * H4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(i % (2 * H4));
        const size_t pos = i / (2 * H4);
        const int b = (int)(pos % Bp), t = (int)(pos / Bp);
        cat[i] = w < H4 ? hf[((size_t)(t + 1) * Bp + b) * H4 + w]
                        : hb[((size_t)(rev_t(t, len[b]) + 1) * Bp + b) * H4 + (w - H4)];
    }
}
hipError_t launch_cat_outputs(hipStream_t s, const float* hs_f, const float* hs_b, const int* len, float* cat, int T, int Bp, int Hp) {
    const size_t total = (size_t)T * Bp * 2 * (Hp / 4);
    cat_outputs_kernel<<<(int)min((size_t)4096, (total + 255) / 256), 256, 0, s>>>((const f32x4*)hs_f, (const f32x4*)hs_b, len,
                                                                                 (f32x4*)cat, T, Bp, Hp / 4);
    return hipGetLastError();
}

__global__ void hcat_kernel(const float* __restrict__ hf, const float* __restrict__ hb, float* __restrict__ out, int Bp, int Hp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Bp * 2 * Hp) return;
    const int w = i % (2 * Hp), b = i / (2 * Hp);
    out[i] = w < Hp ? hf[(size_t)b * Hp + w] : hb[(size_t)b * Hp + w - Hp];
}
hipError_t launch_hcat(hipStream_t s, const float* hf, const float* hb, float* out, int Bp, int Hp) {
    hcat_kernel<<<(Bp * 2 * Hp + 255) / 256, 256, 0, s>>>(hf, hb, out, Bp, Hp);
    return hipGetLastError();
}
__global__ void split_cols_kernel(const float* __restrict__ src, float* __restrict__ a, float* __restrict__ b, int rows, int Hp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 2 * Hp) return;
    const int w = i % (2 * Hp), r = i / (2 * Hp);
    if (w < Hp) a[(size_t)r * Hp + w] = src[i]; else b[(size_t)r * Hp + w - Hp] = src[i];
}
hipError_t launch_split_cols(hipStream_t s, const float* src, float* a, float* b, int rows, int Hp) {
    split_cols_kernel<<<(rows * 2 * Hp + 255) / 256, 256, 0, s>>>(src, a, b, rows, Hp);
    return hipGetLastError();
}

__global__ void uncat_kernel(const float* __restrict__ f, const float* __restrict__ r, const int* __restrict__ len,
                             float* __restrict__ out_f, float* __restrict__ out_b, int T, int Bp, int W, int Hp) {
    const size_t total = (size_t)T * Bp * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const size_t pos = i / W;
        const int b = (int)(pos % Bp), t = (int)(pos / Bp);
        const int tr = rev_t(t, len[b]);
        const float d = f[i] + r[((size_t)tr * Bp + b) * W + w];                   // gradient wrt the level's input at time t
        if (!out_b) out_f[i] = d;
        else if (w < Hp) out_f[((size_t)t * Bp + b) * Hp + w] = d;                     // forward direction: its own time
        else out_b[((size_t)tr * Bp + b) * Hp + (w - Hp)] = d;                         // backwards direction: reversed time
    }
}
hipError_t launch_uncat(hipStream_t s, const float* f, const float* r, const int* len, float* out_f, float* out_b, int T, int Bp,
                        int W, int Hp) {
    const size_t total = (size_t)T * Bp * W;
    uncat_kernel<<<(int)min((size_t)4096, (total + 255) / 256), 256, 0, s>>>(f, r, len, out_f, out_b, T, Bp, W, Hp);
    return hipGetLastError();
}

hipError_t launch_gather_xt(hipStream_t s, const float* Win, const float* bias, const int* X, float* xt, int T, int Bp,
                            int F, int GHp, int) {
    const int R4 = GHp / 4;
    const size_t total = (size_t)T * Bp * R4;
    const int grid = (int)min((size_t)256 * 16, (total + 255) / 256);
    gather_xt_kernel<<<grid, 256, 0, s>>>((const f32x4*)Win, (const f32x4*)bias, X, (f32x4*)xt, T, Bp, F, R4);
    return hipGetLastError();
}

// Gate of the overlapped step tail (sbr_backward_recurrent): returns once every wave of the running BPTT chain
// (rec_bwd_x6p<.., WT>) has published a progress word of this launch (epoch) at or below `target`, i.e. once all time
// steps >= target are complete AND written through to memory.  The kernels enqueued behind it on the same stream are
// ordinary consumers of those time steps.  One workgroup; the poll is a relaxed agent-scope load with s_sleep between
// polls; the spin is bounded (fault bit 3, reported with the cost) so that a chain that never starts cannot hang the GPU.
__global__ void __launch_bounds__(512) tail_gate_kernel(const int* __restrict__ progress, int n, int epoch, int target, int* __restrict__ fault) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long t0 = wall_clock64();
        for (;;) {
            const int v = __hip_atomic_load(progress + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((v >> 12) == epoch && (v & 0xfff) <= target) break;
            if (wall_clock64() - t0 > SBR_POLL_TICKS) { atomicOr(fault, 8); break; }
            __builtin_amdgcn_s_sleep(8);
        }
    }
}

// The MONITOR of an overlapped step tail (tail_monitor_loop: workgroup 0 of the LDS-row scatter-add launch; as this kernel on a stream
// of its own where that launch is not taken, and on the one stream of the serial mode): one workgroup folds the chain's per-wave progress words into
// `done` = (epoch << 12) | max t (SBR_DONE_COPIES copies, sbr_common.h SbrPoll) for as long as the chain runs -- relaxed
// agent-scope loads, stores only when the maximum moves -- and leaves when every wave has reached t_lo.  (Rounds 2 / 3a: a
// workgroup of the polling GEMM did this; the consumers then depended on WHEN that launch got onto the chip.)
__global__ void __launch_bounds__(256) tail_monitor_kernel(SbrPoll pl, int t_lo) { tail_monitor_loop(pl, t_lo); }
hipError_t launch_tail_monitor(hipStream_t s, const SbrPoll& poll, int t_lo) {
    tail_monitor_kernel<<<1, 256, 0, s>>>(poll, t_lo);
    return hipGetLastError();
}

hipError_t launch_tail_gate(hipStream_t s, const int* progress, int n, int epoch, int target, int* fault) {
    tail_gate_kernel<<<1, 512, 0, s>>>(progress, n, epoch, target, fault);
    return hipGetLastError();
}

// The same gate for the HEAD of the side stream of a single-call step (sbr_loss_backward_output): it is launched in front of the
// chain and is on the chip while the forward chain and the head run, so it is one wave without LDS.  Until the chain appears
// it polls ONE word, kTailGateSleep sleep units apart (a load per microsecond); then its lanes read all n words at once,
// eight loads in flight each, until every one is of this epoch.  A word of this epoch means that the chain has started, i.e. that
// everything in front of it on the main stream is complete and written back; a word the step before left carries the epoch
// before.  The bound and the fault bit are tail_gate_kernel's: a chain that never comes (an error return between the two
// phases) ends the wait by itself.
__global__ void __launch_bounds__(64) tail_gate_wave_kernel(const int* __restrict__ progress, int n, int epoch, int target, int* __restrict__ fault) {
    const unsigned long long t0 = wall_clock64();
    auto passed = [&](int v) { return (v >> 12) == epoch && (v & 0xfff) <= target; };
    for (;;) {
        if (passed(__hip_atomic_load(progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) break;
        if (wall_clock64() - t0 > SBR_POLL_TICKS) { if (threadIdx.x == 0) atomicOr(fault, 8); return; }
        __builtin_amdgcn_s_sleep(kTailGateSleep);
    }
    for (;;) {
        bool ok = true;
#pragma unroll 8
        for (int i = 0; i < n; i += 64)      // (uniform trip count, the index clamped: nothing between the loads)
            ok = passed(__hip_atomic_load(progress + min(i + (int)threadIdx.x, n - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) && ok;
        if (__all(ok)) break;
        if (wall_clock64() - t0 > SBR_POLL_TICKS) { if (threadIdx.x == 0) atomicOr(fault, 8); return; }
        __builtin_amdgcn_s_sleep(8);
    }
}
hipError_t launch_tail_gate_wave(hipStream_t s, const int* progress, int n, int epoch, int target, int* fault) {
    if (n < 1) return hipErrorInvalidValue;
    tail_gate_wave_kernel<<<1, 64, 0, s>>>(progress, n, epoch, target, fault);
    return hipGetLastError();
}

// Gate of the step boundary (sbr_step.hip: the join of the consumer streams at the end of a single-call step with the overlapped
// tail, the release of the second side stream and of the batch builder at its start): one wave, no LDS, returns once w0[0] (and
// w1[0], where given) hold `epoch`.  The words are stored write-through by kernels that were enqueued BEFORE this one
// (step_word_kernel behind the last kernel of a consumer stream; the forward chain's entry: RecArgs.start_word), so the wait ends
// by itself; the bound and the fault bit are tail_gate_kernel's all the same.  Relaxed agent-scope loads, s_sleep between polls;
// what is enqueued behind the gate sees the publishers' data through its own kernel-start acquire.
__global__ void __launch_bounds__(64) step_gate_kernel(const int* __restrict__ w0, const int* __restrict__ w1, int epoch, int* __restrict__ fault) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        const int a = __hip_atomic_load(w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int b = w1 ? __hip_atomic_load(w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
        if (a == epoch && b == epoch) break;
        if (wall_clock64() - t0 > SBR_POLL_TICKS) { if (threadIdx.x == 0) atomicOr(fault, 8); return; }
        __builtin_amdgcn_s_sleep(8);
    }
}
hipError_t launch_step_gate(hipStream_t s, const int* w0, const int* w1, int epoch, int* fault) {
    if (!w0 || !epoch) return hipErrorInvalidValue;
    step_gate_kernel<<<1, 64, 0, s>>>(w0, w1, epoch, fault);
    return hipGetLastError();
}
// The completion word of a stream: one lane stores `epoch`, write-through, as the first thing it does.  That this kernel has
// started means that everything in front of it on its stream is complete and written back (the argument of tail_gate_wave_kernel
// above and of RecArgs.start_word) -- the release is the one the queue makes at the end of every kernel, once, for all XCDs.
__global__ void __launch_bounds__(64) step_word_kernel(int* __restrict__ word, int epoch) {
    if (threadIdx.x == 0) __hip_atomic_store(word, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
hipError_t launch_step_word(hipStream_t s, int* word, int epoch) {
    if (!word || !epoch) return hipErrorInvalidValue;
    step_word_kernel<<<1, 64, 0, s>>>(word, epoch);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// K8 full softmax + categorical cross-entropy, forward and backward fused, one workgroup per
// row (rnn_one_hot.py:65-71): in: raw h.W_out; out (in place): dcost/dlogits.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) softmax_cce_kernel(float* __restrict__ logits, const float* __restrict__ bout,
                                                          const int* __restrict__ target, const float* __restrict__ pop,
                                                          float* __restrict__ rowcost, int N, long ld, int Bglobal) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    float* x = logits + (size_t)r * ld;
    float mx = -INFINITY;
    for (int n = threadIdx.x; n < N; n += 256) { const float v = x[n] + bout[n]; x[n] = v; mx = fmaxf(mx, v); }
    mx = block_max(mx, red);
    float se = 0.0f;
    for (int n = threadIdx.x; n < N; n += 256) se += expf(x[n] - mx);
    se = block_sum(se, red);
    const int y = target[r];
    const float scale = 1.0f / (pop[r] * (float)Bglobal);
    const float xy = x[y];
    __syncthreads();
    const float inv = 1.0f / se;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float p = expf(x[n] - mx) * inv;
        x[n] = (p - (n == y ? 1.0f : 0.0f)) * scale;
    }
    if (threadIdx.x == 0) rowcost[r] = (logf(se) + mx - xy) * scale;
}

// Same, with the row held in LDS (N * 4 bytes <= ~150 KB, i.e. catalogues up to ~38 k items): one read and one write
// of the logits instead of three reads and two writes, 1024 threads per row, hardware exp2.  C4 (N = 26744): 133 -> ~30 us.
__global__ void __launch_bounds__(1024) softmax_cce_lds_kernel(float* __restrict__ logits, const float* __restrict__ bout,
                                                               const int* __restrict__ target, const float* __restrict__ pop,
                                                               float* __restrict__ rowcost, int N, long ld, int Bglobal) {
    extern __shared__ float row[];
    __shared__ float red[16];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* x = logits + (size_t)r * ld;
    float mx = -INFINITY;
    for (int n = tid; n < N; n += 1024) { const float v = x[n] + bout[n]; row[n] = v; mx = fmaxf(mx, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
    __syncthreads();
    float se = 0.0f;
    for (int n = tid; n < N; n += 1024) { const float e = __builtin_amdgcn_exp2f((row[n] - mx) * 1.4426950408889634f); row[n] = e; se += e; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    if (lane == 0) red[wv] = se;
    const int y = target[r];
    const float scale = 1.0f / (pop[r] * (float)Bglobal);
    __syncthreads();
    se = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) se += red[w];                 // fixed order: deterministic
    const float inv = 1.0f / se;
    // cost = log(se) + mx - x_y with x_y recovered from e_y = exp(x_y - mx): keep it exact instead: re-read the logit
    const float xy = x[y] + bout[y];
    __syncthreads();                                           // everyone has read x[y] before the row is overwritten
    for (int n = tid; n < N; n += 1024) x[n] = (row[n] * inv - (n == y ? 1.0f : 0.0f)) * scale;
    if (tid == 0) rowcost[r] = (logf(se) + mx - xy) * scale;
}

hipError_t launch_softmax_cce(hipStream_t s, float* logits, const float* bout, const int* target, const float* pop,
                              float* rowcost, int rows, int N, long ld, int Bglobal) {
    if (rows <= 0) return hipSuccess;
    const size_t lds = (size_t)N * sizeof(float);
    if (lds <= 150 * 1024) {
        SBR_DYN_LDS(softmax_cce_lds_kernel, lds);
        softmax_cce_lds_kernel<<<rows, 1024, lds, s>>>(logits, bout, target, pop, rowcost, N, ld, Bglobal);
        return hipGetLastError();
    }
    softmax_cce_kernel<<<rows, 256, 0, s>>>(logits, bout, target, pop, rowcost, N, ld, Bglobal);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// RNNMargin's multi-target losses (rnn_margin.py:62-69), forward and backward fused, one workgroup per row.
// The reference builds dense (B, N) target / weight matrices on the host (:112-147); here a row is: the default target
// and the false-positive weight w = balance * n_pos / (N - n_pos - n_in) everywhere, then the overrides, few entries each
// and possibly repeated: the positives (target 1, weight -1), and LAST -- with unique interactions -- the row's input
// items (target 0, weight 0; an input item that is also a positive ends there).  The overridden logits are put aside
// before the dense pass overwrites the row with gradients; duplicates are recognised by comparing against the earlier
// entries (k <= T + NT entries in LDS).   loss / d loss / d p of one element:
//   hinge   relu((p - y) w)               | w if (p - y) w > 0
//   logit   sigmoid(p - y) w              | s (1 - s) w
//   logsig  -log(sigmoid((y - p) w))      | w (1 - sigmoid((y - p) w))
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void margin_elem(int loss, float p, float y, float w, float& l, float& g) {
    if (loss == SBR_LOSS_HINGE) { const float z = (p - y) * w; l = fmaxf(z, 0.0f); g = z > 0.0f ? w : 0.0f; }
    else if (loss == SBR_LOSS_LOGIT) { const float s = 1.0f / (1.0f + expf(y - p)); l = s * w; g = s * (1.0f - s) * w; }
    else { const float z = (y - p) * w; l = fmaxf(-z, 0.0f) + log1pf(expf(-fabsf(z))); g = w * (1.0f - 1.0f / (1.0f + expf(-z))); }
}

__global__ void __launch_bounds__(256) margin_loss_kernel(float* __restrict__ logits, const float* __restrict__ bout,
                                                          const int* __restrict__ target, int NT, const int* __restrict__ X,
                                                          const int* __restrict__ len, int T, int F, const float* __restrict__ dflt,
                                                          float* __restrict__ rowcost, int N, long ld, int Bglobal, int loss,
                                                          float balance, int unique) {
    extern __shared__ int m_ids[];                 // [NT + T] ids of the override entries, then their logits (floats)
    __shared__ float red[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    float* x = logits + (size_t)r * ld;
    float* m_p = (float*)(m_ids + NT + T);
    const int n_in = len[r];
    int nt = 0;
    for (int j = 0; j < NT; ++j) nt += target[(size_t)r * NT + j] >= 0 ? 1 : 0;
    const int k = nt + (unique ? n_in : 0);
    for (int e = tid; e < k; e += 256) {
        const int id = e < nt ? target[(size_t)r * NT + e] : X[((size_t)r * T + (e - nt)) * F];
        m_ids[e] = id;
        m_p[e] = x[id] + bout[id];
    }
    __syncthreads();
    const float w_fp = balance * (float)nt / (float)(N - nt - n_in);
    const float inv = 1.0f / (float)Bglobal;
    float acc = 0.0f;
    for (int n = tid; n < N; n += 256) {
        float l, g;
        margin_elem(loss, x[n] + bout[n], dflt ? dflt[n] : 0.0f, w_fp, l, g);
        x[n] = g * inv;
        acc += l;
    }
    __syncthreads();
    for (int e = tid; e < k; e += 256) {
        const int id = m_ids[e];
        const bool seen = e >= nt;
        bool dup = false;
        for (int f = seen ? nt : 0; f < e; ++f) dup = dup || m_ids[f] == id;         // an earlier entry of the same kind
        if (!seen && unique) for (int f = nt; f < k; ++f) dup = dup || m_ids[f] == id;   // a positive that is also an input item
        if (dup) continue;
        float l0, g0, l1, g1;
        margin_elem(loss, m_p[e], dflt ? dflt[id] : 0.0f, w_fp, l0, g0);
        margin_elem(loss, m_p[e], seen ? 0.0f : 1.0f, seen ? 0.0f : -1.0f, l1, g1);
        x[id] = g1 * inv;
        acc += l1 - l0;
    }
    acc = block_sum(acc, red);
    if (tid == 0) rowcost[r] = acc * inv;
}

hipError_t launch_margin_loss(hipStream_t s, float* logits, const float* bout, const int* target, int NT, const int* X,
                              const int* len, int T, int F, const float* dflt, float* rowcost, int rows, int N, long ld,
                              int Bglobal, int loss, float balance, int unique) {
    if (rows <= 0) return hipSuccess;
    const size_t lds = (size_t)(NT + T) * (sizeof(int) + sizeof(float));
    SBR_DYN_LDS(margin_loss_kernel, lds);
    margin_loss_kernel<<<rows, 256, lds, s>>>(logits, bout, target, NT, X, len, T, F, dflt, rowcost, N, ld, Bglobal, loss, balance, unique);
    return hipGetLastError();
}

// predict path: x += b, optional softmax (rnn_base.py:188-194, rnn_sampling.py:144)
__global__ void __launch_bounds__(256) softmax_rows_kernel(float* __restrict__ logits, const float* __restrict__ bout, int N,
                                                           int do_softmax) {
    __shared__ float red[4];
    float* x = logits + (size_t)blockIdx.x * N;
    float mx = -INFINITY;
    for (int n = threadIdx.x; n < N; n += 256) { const float v = x[n] + bout[n]; x[n] = v; mx = fmaxf(mx, v); }
    if (!do_softmax) return;
    const float inv = softmax_row_scale(x, N, mx, red, mx);      // (sbr_device.h: cev_product_kernel takes the same two calls)
    for (int n = threadIdx.x; n < N; n += 256) x[n] = softmax_row_value(x[n], mx, inv);
}

hipError_t launch_softmax_rows(hipStream_t s, float* logits, const float* bout, int rows, int N, int do_softmax) {
    if (rows <= 0) return hipSuccess;
    softmax_rows_kernel<<<rows, 256, 0, s>>>(logits, bout, N, do_softmax);
    return hipGetLastError();
}

// db[n] = sum_r d[r][n] (+ d reg/db); rnn_one_hot.py:73-77 regularises the output bias only.
// Two stages (rows split over gridDim.y, partials summed in fixed order): deterministic, and
// enough workgroups to stream the (rows, N) matrix at HBM speed.
#define COLSUM_SPLIT 16
__global__ void colsum_partial_kernel(const float* __restrict__ d, int rows, int N, long ld, float* __restrict__ part) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int per = (rows + COLSUM_SPLIT - 1) / COLSUM_SPLIT;
    const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
    float s = 0.0f;
    for (int r = r0; r < r1; ++r) s += d[(size_t)r * ld + n];
    part[(size_t)blockIdx.y * N + n] = s;
}
__global__ void colsum_bias_kernel(const float* __restrict__ part, int N, float* __restrict__ db,
                                   const float* __restrict__ b, float reg) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < COLSUM_SPLIT; ++k) s += part[(size_t)k * N + n];
    if (reg > 0.0f) s += 2.0f * reg * b[n];
    else if (reg < 0.0f) s -= reg * (b[n] > 0.0f ? 1.0f : (b[n] < 0.0f ? -1.0f : 0.0f));
    db[n] = s;
}
// cost += reg * sum(b^2)  or  |reg| * sum|b|   (single workgroup, fixed order)
__global__ void __launch_bounds__(256) reg_cost_kernel(const float* __restrict__ b, int N, float reg, float* cost) {
    __shared__ float red[4];
    float s = 0.0f;
    for (int n = threadIdx.x; n < N; n += 256) s += reg > 0.0f ? b[n] * b[n] : fabsf(b[n]);
    s = block_sum(s, red);
    if (threadIdx.x == 0) *cost += fabsf(reg) * s;
}

hipError_t launch_colsum_bias(hipStream_t s, const float* d, int rows, int N, long ld, float* db, const float* b,
                              float reg, float* cost, float* ws) {
    colsum_partial_kernel<<<dim3((N + 255) / 256, COLSUM_SPLIT), 256, 0, s>>>(d, rows, N, ld, ws);
    colsum_bias_kernel<<<(N + 255) / 256, 256, 0, s>>>(ws, N, db, b, reg);
    if (reg != 0.0f && cost) reg_cost_kernel<<<1, 256, 0, s>>>(b, N, reg, cost);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) sum_cost_kernel(const float* __restrict__ rowcost, int rows, float* cost) {
    __shared__ float red[4];
    float s = 0.0f;
    for (int r = threadIdx.x; r < rows; r += 256) s += rowcost[r];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *cost = s;
}
hipError_t launch_sum_cost(hipStream_t s, const float* rowcost, int rows, float* cost) {
    sum_cost_kernel<<<1, 256, 0, s>>>(rowcost, rows, cost);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Sampled heads (BlackoutLayer, sparse_lstm.py:42-54; losses rnn_sampling.py:68-91)
// ---------------------------------------------------------------------------------------
__global__ void build_cells_kernel(const int* target, const int* samples, int Bg, int S, int* cells) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < Bg + S) cells[c] = c < Bg ? target[c] : samples[c - Bg];   // T.concatenate((targets, output_cells)) :50
}
hipError_t launch_build_cells(hipStream_t s, const int* target, const int* samples, int Bg, int S, int* cells) {
    build_cells_kernel<<<(Bg + S + 255) / 256, 256, 0, s>>>(target, samples, Bg, S, cells);
    return hipGetLastError();
}

// W_out is stored item-major [N][Hp], so W[:, cells] (sparse_lstm.py:52) is a coalesced row gather
__global__ void gather_rows_kernel(const f32x4* __restrict__ W, const float* __restrict__ b, const int* __restrict__ cells,
                                   int C, int R4, f32x4* __restrict__ Wc, float* __restrict__ bc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * R4) return;
    const int c = i / R4, f4 = i % R4;
    Wc[i] = W[(size_t)cells[c] * R4 + f4];
    if (f4 == 0) bc[c] = b[cells[c]];
}
hipError_t launch_gather_rows(hipStream_t s, const float* W, const float* b, const int* cells, int C, int Hp, float* Wc,
                              float* bc) {
    const int R4 = Hp / 4;
    gather_rows_kernel<<<(C * R4 + 255) / 256, 256, 0, s>>>((const f32x4*)W, b, cells, C, R4, (f32x4*)Wc, bc);
    return hipGetLastError();
}

__device__ __forceinline__ float sigmf(float x) { return 1.0f / (1.0f + expf(-x)); }

// one workgroup per local row r; act row (C = Bg+S columns) in: h.Wc^T, out: dcost/dact
__global__ void __launch_bounds__(256) sampled_loss_kernel(float* __restrict__ act, const float* __restrict__ bc,
                                                           const float* __restrict__ pop, float* __restrict__ rowcost,
                                                           int Bg, int S, int row_offset, int loss, int Bglobal) {
    __shared__ float red[4];
    const int r = blockIdx.x, C = Bg + S, pos = row_offset + r;
    float* a = act + (size_t)r * C;
    const float scale = 1.0f / (pop[r] * (float)Bglobal);
    if (bc) { for (int c = threadIdx.x; c < C; c += 256) a[c] += bc[c]; }      // + b[output_cells] :54 (the cluster head's scores have none)
    __syncthreads();
    const float apos = a[pos];
    float L;
    if (loss == SBR_LOSS_BLACKOUT || loss == SBR_LOSS_SCCE) {         // rnn_sampling.py:68-72; SCCE: rnn_cluster.py:158-162
        const bool blackout = loss == SBR_LOSS_BLACKOUT;
        float mx = -INFINITY;
        for (int c = threadIdx.x; c < C; c += 256) mx = fmaxf(mx, a[c]);
        mx = block_max(mx, red);
        float se = 0.0f;
        for (int c = threadIdx.x; c < C; c += 256) se += expf(a[c] - mx);
        se = block_sum(se, red);
        const float inv = 1.0f / se;
        const float ppos = expf(apos - mx) * inv;
        // sum_k dLdp_k p_k  and  sum of -log(1-p) over the negatives
        float dot = 0.0f, lneg = 0.0f;
        for (int c = threadIdx.x; c < C; c += 256) {
            const float p = expf(a[c] - mx) * inv;
            if (c >= Bg && blackout) { dot += p / (1.0f - p); lneg -= logf(1.0f - p); }
        }
        dot = block_sum(dot, red) - 1.0f;                             // positive: (-1/p_pos) * p_pos
        lneg = block_sum(lneg, red);
        L = -logf(ppos) + lneg;
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const float p = expf(a[c] - mx) * inv;
            float dldp = 0.0f;
            if (c >= Bg && blackout) dldp = 1.0f / (1.0f - p);
            if (c == pos) dldp += -1.0f / p;
            a[c] = p * (dldp - dot) * scale;
        }
    } else {
        float lsum = 0.0f, dpos = 0.0f;
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            if (c == pos) continue;                                   // written after the reduction
            float da = 0.0f;
            if (c >= Bg) {
                const float v = a[c], diff = v - apos;
                if (loss == SBR_LOSS_BPR) {                           // :80-84  -log(sigmoid(-diff)) = softplus(diff)
                    lsum += fmaxf(diff, 0.0f) + log1pf(expf(-fabsf(diff)));
                    const float dd = sigmf(diff) / (float)S;
                    da = dd; dpos += dd;
                } else if (loss == SBR_LOSS_BPRELU) {                 // rnn_cluster.py:173-175: leaky_rectify(diff + 0.5), leakiness 0.01 [3P]
                    const float yv = diff + 0.5f;
                    lsum += yv > 0.0f ? yv : 0.01f * yv;
                    const float dd = (yv > 0.0f ? 1.0f : 0.01f) / (float)S;
                    da = dd; dpos += dd;
                } else if (loss == SBR_LOSS_LIN) {                    // rnn_cluster.py:164-167: SUM of the negatives - the positive
                    lsum += v;
                    da = 1.0f;
                } else {                                              // TOP1 :86-91
                    const float s1 = sigmf(diff), s2 = sigmf(v * v);
                    lsum += s1 + s2;
                    const float d1 = s1 * (1.0f - s1) / (float)S;
                    da = d1 + s2 * (1.0f - s2) * 2.0f * v / (float)S; dpos += d1;
                }
            }
            a[c] = da * scale;
        }
        lsum = block_sum(lsum, red);
        dpos = block_sum(dpos, red);
        L = lsum / (float)S;
        if (loss == SBR_LOSS_LIN) { L = lsum - apos; dpos = 1.0f; }
        if (threadIdx.x == 0) a[pos] = -dpos * scale;
    }
    if (threadIdx.x == 0) rowcost[r] = L * scale;
}

hipError_t launch_sampled_loss(hipStream_t s, float* act, const float* bc, const float* pop, float* rowcost, int rows,
                               int Bg, int S, int row_offset, int loss, int Bglobal) {
    if (rows <= 0) return hipSuccess;
    sampled_loss_kernel<<<rows, 256, 0, s>>>(act, bc, pop, rowcost, Bg, S, row_offset, loss, Bglobal);
    return hipGetLastError();
}

// dW_out^T[cells[c]][:] += dWc[c][:], db_out[cells[c]] += dbc[c]; duplicates accumulate [3P]
__global__ void scatter_cells_kernel(float* __restrict__ dW, float* __restrict__ db, const float* __restrict__ dWc,
                                     const float* __restrict__ dbc, const int* __restrict__ cells, int C, int Hp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * Hp) return;
    const int c = i / Hp, k = i % Hp;
    atomicAdd(&dW[(size_t)cells[c] * Hp + k], dWc[i]);
    if (k == 0) atomicAdd(&db[cells[c]], dbc[c]);
}
hipError_t launch_scatter_cells(hipStream_t s, float* dW, float* db, const float* dWc, const float* dbc, const int* cells,
                                int C, int Hp) {
    scatter_cells_kernel<<<(C * Hp + 255) / 256, 256, 0, s>>>(dW, db, dWc, dbc, cells, C, Hp);
    return hipGetLastError();
}

__global__ void fill_kernel(float* p, float v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
hipError_t launch_fill(hipStream_t s, float* p, float v, size_t n) {
    const int grid = (int)min((size_t)256 * 16, (n + 255) / 256);
    fill_kernel<<<grid, 256, 0, s>>>(p, v, n);
    return hipGetLastError();
}
