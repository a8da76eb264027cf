// Internal declarations shared by the HIP translation units of libsbr_rnn.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <string>
#include <vector>
#include "../../include/sbr_rnn.h"
#include "sbr_upd.h"

#define SBR_BWD_CHUNKS 4       // BPTT launches per layer when T >= 64 (bf16x6 kernels)
#define SBR_ALIGN_FLOATS 64   // every carved buffer starts on a 256-byte boundary

static inline size_t sbr_align(size_t n_floats) { return (n_floats + SBR_ALIGN_FLOATS - 1) / SBR_ALIGN_FLOATS * SBR_ALIGN_FLOATS; }
static inline int sbr_gates(int cell) { return cell == SBR_CELL_LSTM ? 4 : (cell == SBR_CELL_GRU ? 3 : 1); }
// Hidden size padded for the MFMA tiling: 16/32/64/128 (W_hid register-resident single-workgroup kernels), 256 for
// anything in (128, 256] and 512 for (256, 512] (the cluster kernels of sbr_rec_cl.hip: a 150-wide layer padded to 256
// runs ~6x faster there than at 192 on the streamed f32 kernels), above that the next multiple of 64 (streamed-W kernels).
static inline int sbr_pad_hidden(int H) {
    if (H <= 16) return 16;
    if (H <= 32) return 32;
    if (H <= 64) return 64;
    if (H <= 128) return 128;
    if (H <= 256) return 256;
    if (H <= 512) return 512;
    return (H + 63) / 64 * 64;
}

// ---------------------------------------------------------------------------------------
// Parameter / activation layout in the device arena (all float32, offsets in floats)
// ---------------------------------------------------------------------------------------
struct LayerLayout {
    int H, Hp, G;
    int n_in;        // logical rows of W_in (input_size for layer 0, H of the layer below otherwise)
    int n_in_p;      // stored rows (== n_in for layer 0, Hp of the layer below otherwise)
    // parameter section offsets (the gradient section mirrors them exactly)
    size_t p_Win;    // [n_in_p][G*Hp]   item-major rows, gate-major inside a row
    size_t p_b;      // [G*Hp]
    size_t p_Whid;   // [Hp][G*Hp]
    size_t p_peep;   // [3][Hp]          LSTM only (i, f, o)
    size_t p_cinit;  // [Hp]             LSTM only
    size_t p_hinit;  // [Hp]
    // activation offsets (activation section)
    size_t a_xt;     // [T][Bp][G*Hp]    precomputed input (gather or dense GEMM)
    size_t a_hs;     // [T+1][Bp][Hp]    slot 0 = hid_init, slot t+1 = h_t
    size_t a_cs;     // [T+1][Bp][Hp]    LSTM cell states
    size_t a_xh, a_pring;   // wide layers (Hp = 256 / 512): exchange arrays of the 16-row cluster kernels, else 0
    size_t a_g[4];   // [T][Bp][Hp]      LSTM i,f,g,o / GRU r,u,c~,hid_c
    size_t a_dxt;    // [T][Bp][G*Hp]    grad wrt xt (= grad wrt gates for LSTM/Vanilla)
    size_t a_dhi;    // [T][Bp][Hp]      GRU only: candidate-gate slice of grad wrt hid_input (r,u slices equal dxt)
    size_t a_dhext;  // [T][Bp][Hp]      grad arriving from the layer above (layers below the top)
    size_t a_state;  // [2][Bp][Hp] dh, dc carried between BPTT chunk launches
    size_t a_part;   // [SBR_BWD_CHUNKS][Bp][G*Hp + 5*Hp] per-workgroup partial sums (up to one workgroup per row): bias, peepholes, inits
};

// A row-sparse parameter block: rows of up to two arrays that are touched together (the forward and backwards layer-0
// W_in under --r_bi; W_out^T and b_out of a sampled head) share one row index space and one `last` array.
struct SparseBlockLayout {
    int kind;            // 0: rows indexed by the batch's input ids (layer-0 W_in or the embedding table); 1: by the sampled cells
    int npairs;
    size_t off[2];       // offset of row 0 inside the parameter / gradient / state sections
    int width[2];        // floats of a row that are stored there
    int stride[2];       // floats between consecutive rows
    int n_rows;
    int W;               // packed row width (sum of the widths) in the exchange buffers
    int max_local;       // most rows one rank can touch per step (capacity of its exchange buffers)
    size_t a_last;       // [n_rows] ints: step through which the row is current
    size_t a_mark;       // [n_rows] ints: pack epoch (dedupe of the exchange)
    size_t a_cand;       // [cand_cap] ints: the step's candidate rows in a data-parallel step (ids of every rank)
    size_t a_count;      // device int: rows packed by the last sbr_sparse_pack
    int cand_cap;
};

struct Layout {
    sbr_config cfg;
    int n_sparse;                         // row-sparse blocks (0: every parameter takes the dense update)
    SparseBlockLayout sparse[2];
    size_t a_at; int n_at; int adam_early_exit;   // adam's a_t table (floats) for the lazy catch-up
    int L, G, T, B, Bp, N, F, Bg, S, C;   // C = Bg + S sampled columns
    int HLp;                              // padded width of one direction of the top layer
    int D, HLt;                           // directions per level (2 with --r_bi) and the output layer's input width D * HLp
    // --r_bi only (the backwards direction runs the ordinary kernels on per-row time-reversed copies of its input):
    size_t a_Xr;                          // [Bp][T][F] ints: item ids reversed inside each row's valid length
    size_t a_embr;                        // [T][Bp][F*Ep] reversed flattened embeddings (--r_emb)
    size_t a_cat[SBR_MAX_LAYERS], a_catr[SBR_MAX_LAYERS];   // [T][Bp][2*Hp_l] concatenated outputs of level l (forward time / reversed)
    size_t a_hcat;                        // [Bp][2*HLp] final states of both directions
    size_t a_dhl[2];                      // [Bp][HLp] halves of dh_last
    size_t a_dinp[2];                     // [T][Bp][max dense n_in_p] gradient wrt a dense level's input, per direction
    size_t a_s2cnt, a_s2off, a_s2cur, a_s2sid, a_s2pos;     // scatter sort workspace of the reversed ids
    int E, Ep;                            // --r_emb: embedding width and its stored width (multiple of 4); 0 = none
    size_t p_Emb;                         // [input_size][Ep]
    size_t a_emb, a_demb;                 // [T][Bp][F*Ep] flattened embeddings = dense input of layer 0, and its gradient
    LayerLayout layer[2 * SBR_MAX_LAYERS];   // [l * D + d]: d = 0 forward, 1 backwards (--r_bi)
    size_t p_WoutT, p_bout;               // [N][HLp], [N]
    size_t n_params;                      // floats in the parameter section
    size_t p_split;                       // == p_WoutT : output-layer part starts here
    size_t n_state_arrays;                // optimizer state arrays of n_params floats each (1 or 2)
    // arena sections (float offsets from the arena base)
    size_t s_params, s_grads, s_state, s_act, s_end;
    // misc activation-section buffers
    size_t a_logits;                      // [Bp][Nl], Nl = N rounded up to 4 floats in the training step (16-byte rows for the
                                          // bf16x6 GEMMs that read dlogits); [rows][N] in predict / top-k
    size_t a_dhlast;                      // [Bp][HLp]
    size_t a_rowcost;                     // [Bp]
    int NT;                               // RNNMargin: target columns per row (1 for the other heads)
    size_t a_dflt;                        // RNNMargin: [N] default target (zeros unless sbr_set_default_target)
    size_t a_Wc, a_bc, a_act, a_dWc, a_dbc; // sampled heads: [C][HLp], [C], [Bp][C], [C][HLp], [C]
    size_t a_ws; size_t ws_floats;        // split-K workspace (main stream)
    size_t a_ws2; size_t ws2_floats;      // split-K workspace of the side stream (output-layer + weight gradients)
    size_t a_csum;                        // [16][max(N,C)] column-sum partials
    size_t a_prof;                        // [2][nblk][16][4] uint64 in-kernel cycle counters (fwd, bwd)
    size_t a_fault;                       // int: a cluster exchange wait timed out
    size_t a_clx;                         // cluster handshake slots (ints)
    size_t a_X, a_len, a_tgt, a_smp, a_cells, a_pop, a_topk; // batch buffers (ints stored in float slots)
    size_t a_X2, a_len2, a_tgt2, a_smp2, a_pop2;             // ... second set: sbr_build_batch fills the set the step in flight does not read
    size_t a_scnt, a_soff, a_scur, a_sid, a_spos;            // scatter counting-sort workspace (ints)
    size_t a_sP;                          // [input_size + 1] running cost of the ids (launch_scatter_lds_poll)
    size_t a_hstat;                       // [256][16][4] row statistics the chunks of the fused head exchange (sbr_head.hip)
    size_t a_srpart, a_srid; int sr_slots;   // scatter-add of wide rows: partial rows of the long segments' pieces, counters + records (0: not used)
    int tail_keys;                        // time chunks the sort's key space was sized for (1: no tail overlap possible)
    size_t a_prog;                        // [Bp / 4 * 8] progress words of the running BPTT chain (tail overlap)
    size_t a_done;                        // [SBR_DONE_COPIES * SBR_DONE_STRIDE] the monitor's word (the minimum over a_prog), replicated
};

int sbr_build_layout(const sbr_config& cfg, Layout& lay, std::string& err);

struct ParamDesc { std::string name; int layer; int kind; int gate; int64_t d0, d1; int ndim; };
// kind: 0 W_in, 1 W_hid, 2 b, 3 peephole(i,f,o by gate 0..2), 4 cell_init, 5 hid_init, 6 out.W, 7 out.b
void sbr_param_descs(const Layout& lay, std::vector<ParamDesc>& out);

// Time chunks of the time-chunked sort (overlapped step tail): chunk c holds the time steps [lo[c], lo[c + 1]), n chunks;
// n <= 1: plain keys.  The chunks need not be equal: the BPTT chain completes chunk 0 last, and whatever of the scatter-add
// belongs to it can only start at the chain's end -- so the chunks shrink geometrically towards t = 0.
#define SBR_TCHUNKS_MAX 9
struct SbrTChunks { int n; int lo[SBR_TCHUNKS_MAX + 1]; };
// ---------------------------------------------------------------------------------------
// Tuned constants of the step.  Each was an environment switch while it was being measured (rounds 1 - 5) and is fixed since
// round 6; the A/B numbers are in profiles/round2_b_tail_variants.txt, round3_*_variants.txt, round4_variants.txt,
// round5_variants.txt and DESIGN.md sections 3, 3a, 3d.  The variants that measured slower are gone with their switches: the
// output layer's gradient kernels on a stream of their own (round 4, calls n, q), the unsplit gate math on 4-row tiles, the
// f32 weight-gradient kernel at 128 units, the sort behind the output phase, dh_last reduced in front of rec_bwd_x6p, the
// W_hid slab reduction apart from its update, the unswapped tail of a single-layer step.
// ---------------------------------------------------------------------------------------
constexpr int kWgradSlices = 256;         // K-slices of the weight-gradient kernel (total over the BPTT chunks)
constexpr int kWgradX6Wgs = 512;          // ... of which the bf16x6 GEMM (128 x 128 tiles) takes as many as give ~512 workgroups in all
constexpr int kTailChunksMax = 8;         // overlapped tail: time chunks of the sort's keys, at most
constexpr int kTailPubEvery = 2;          // time steps between two progress words of a chain wave
constexpr int kTailShortChunks = 3;       // time chunks (from t = 0) whose scatter-add entries are cut into short pieces (polling range form)
constexpr int kTailFenceKb = 124;         // LDS the chains claim while consumers / the sort run beside them
constexpr int kTailFirst = 6;             // LDS-row scatter-add: time steps of the last time chunk (~8 entries per unit)
constexpr int kTailScatterUnits = 192;    // ... and its workgroups (the CUs the chain leaves free at C2)
constexpr int kTailGemmGroups = 64;       // persistent groups of the polling dW_hid GEMM (one partial each)
constexpr int kTailSlabMax = 512;         // rows of its largest K slab
constexpr double kTailSlabGrowth = 0.35;  // k steps of a slab per time step of lead (sbr_tail_slab_table)
// the side stream of a single-call step (profiles/tail_release_variants.txt):
constexpr bool kTailGateFirst = true;     // released by the chain's progress words (a one-wave gate at its head) instead of a main-stream record
constexpr int kTailGateSleep = 32;        // ... whose polls of ONE word are this many s_sleep units (64 clocks each) apart until the chain appears
// the boundary between two such steps (profiles/step_boundary_variants.txt): no event on the main stream
constexpr bool kStepJoinGate = true;      // step end: a one-wave gate on the completion words of the two consumer streams joins them
constexpr bool kStepForkGate = true;      // step start: the second side stream (and the batch builder) wait for the forward chain's start word
// growth of the small time chunks near t = 0 (plan_tail, sbr_step.hip): 6, 10, 15, 25 steps for the LDS-row scatter-add, which
// walks them one after the other; 1, 3, 7, 18 for the polling range form
static inline double sbr_tail_geom(int scatter_lds) { return scatter_lds ? 1.6 : 2.6; }

// ScatPlan: the form of the scatter-add of layer 0's index-input gradient and its launch recipe, chosen once per engine (sbr_scat_plan,
// sbr_scatter.hip, called by sbr_create).  ScatForm's values are what sbr_query "scatter_form" reports: sorted
// segment reduce, range form, segment-parallel form, per-element atomics; in an overlapped tail the polling reduce or the LDS rows.
enum ScatForm { SCAT_REDUCE = 0, SCAT_RANGE = 1, SCAT_WIDE = 2, SCAT_ATOMIC = 3, SCAT_POLL = 4, SCAT_LDS = 5 };
struct ScatReduce { int nv; bool comb; };      // form 0's recipe: 16-byte pieces per lane; the combining kernel or the walk (nv 0: no kernel)
struct ScatPlan {
    ScatForm plain = SCAT_REDUCE, tail = SCAT_POLL;      // over the plain-key sort (or without a sort): 0 .. 3; inside an overlapped tail: 4 or 5
    ScatReduce reduce = {0, false};   // form 0, also for the rows of an embedding table in front of layer 0 (emb_grad_scatter)
    int range_nv = 0, wide_nvw = 0, wide_nvb = 0;      // form 1: pieces per thread; form 2: per lane of the heads' waves, per thread of the other two kernels
    int poll_nv = 0;                  // form 4: pieces per lane
    int lds_nv = 0, floor_cost = 0, rows_lds = 0;      // form 5: pieces per lane, cost floor of an id, LDS rows of a unit
    bool wide_rows = false;           // index-input rows of 512 .. 8192 floats with their partial-row slab (forms 1, 2; the row-aware update)
};
// index-input rows that get a partial-row slab (Layout.a_srpart, a_srid); Ep: width of an embedding table in front of layer 0, 0: none
static inline bool sbr_scatter_wide_rows(int Ep, int GHp) { return !Ep && GHp >= 512 && GHp <= 8192; }
// partial-row slots launch_scatter_wide can claim for max_entries sorted entries (the slab has at least as many)
static inline int sbr_scatter_wide_slots(size_t max_entries) { return (int)(max_entries / 64 + max_entries / 65 + 2); }
ScatReduce sbr_scat_reduce_recipe(int row_floats);
ScatPlan sbr_scat_plan(int GHp, int Ep, int n_ids, int entries, int D, bool atomic, int scat_range, int tail_scatter_lds,
                       int tail_chunks, int units, int part_slots);
// sbr_rank (sbr_rank.hip): where its two pairs of regimes change
constexpr int kRankThreads = 1024;        // threads of a row's workgroup in the select and sort kernels (16 waves: one id segment each)
constexpr int kRankLdsRow = 32768;        // longest row whose keys stay in LDS during the select (128 KB of the CU's 160 KB; C4's 26 744 fits)
constexpr int kRankSortLds = 2048;        // largest k the LDS bitonic sort takes (16 KB of 64-bit composites); above: the LSD radix sort in scratch
constexpr int kNextRankSlots = 8;         // sbr_evaluate_positions: positions projected per GEMM launch at the most (consecutive slots of a_hs) ...
constexpr size_t kNextRankScoreBytes = (size_t)64 << 20;   // ... as long as their scores fit this much ranking scratch; one slot otherwise
constexpr int kGoalRankTile = 1024;       // goal items ev_goal_rank_kernel ranks per pass over the row (sbr_eval.hip): one per thread; 8 KB of composites
                                          // + 4 KB of counts beside the 128 KB row = 140.1 KB of the CU's 160 KB
static_assert(kGoalRankTile == kRankThreads, "ev_goal_rank_kernel: a thread owns one goal item of the tile and one word of its scan");

// The order-preserving 32-bit image of a score (sbr_rank.hip's KEY; read by the select kernels there and by ev_goal_rank_kernel):
// sign-flip transform of the float's bits, -0.0 canonicalised to +0.0, NaN and -inf -> 0 = never ranked.
__device__ __forceinline__ unsigned rank_key(float v) {
    if (!(v > -INFINITY)) return 0u;              // NaN, -inf
    unsigned u = __float_as_uint(v);
    if (v == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// How the evaluation reads a user's sequence of L items (test.py:81-83, rnn_base.py:410), the one statement of the rule: items
// [0, half) are viewed, [half, L) are the goal, and the row fed is the window of the last min(T, half) viewed items.  Places count
// from the user's first item; built from the user's two offsets into the dataset's CSR and the engine's T.
struct UserSplit {
    int L, half, fed;
    __host__ __device__ constexpr UserSplit(long long off_lo, long long off_hi, int T)
        : L((int)(off_hi - off_lo)), half(L / 2), fed(T < half ? T : half) {}
    __host__ __device__ constexpr int goal_len() const { return L - half; }
    __host__ __device__ constexpr int viewed_begin() const { return 0; }
    __host__ __device__ constexpr int viewed_end() const { return half; }
    __host__ __device__ constexpr int window_begin() const { return half - fed; }
    __host__ __device__ constexpr int window_end() const { return half; }
};
#define SBR_SPLIT_IS(L, T, H, G, WB) (UserSplit(100, 100 + (L), (T)).half == (H) && UserSplit(100, 100 + (L), (T)).goal_len() == (G) && \
                                      UserSplit(100, 100 + (L), (T)).window_begin() == (WB) && UserSplit(100, 100 + (L), (T)).window_end() == (H))
// (L, T) -> half, goal length, first place of the window; T shorter than, equal to and longer than half
static_assert(SBR_SPLIT_IS(2, 0, 1, 1, 1) && SBR_SPLIT_IS(2, 1, 1, 1, 0) && SBR_SPLIT_IS(2, 5, 1, 1, 0), "L = 2: one item viewed, one the goal");
static_assert(SBR_SPLIT_IS(3, 0, 1, 2, 1) && SBR_SPLIT_IS(3, 1, 1, 2, 0) && SBR_SPLIT_IS(3, 2, 1, 2, 0), "L = 3: the odd item belongs to the goal");
static_assert(SBR_SPLIT_IS(7, 2, 3, 4, 1) && SBR_SPLIT_IS(7, 3, 3, 4, 0) && SBR_SPLIT_IS(7, 4, 3, 4, 0), "L = 7: the window is the END of the viewed half");
#undef SBR_SPLIT_IS

// How sbr_evaluate_positions reads the same sequence x_0 .. x_{L-1}, the one statement of that rule: the row fed is the
// first fed = min(L - 1, T) items, FROM THE START of the sequence -- not the window of the viewed half --, and every position
// p = min_history .. fed is evaluated: the state is slot p of the top layer's a_hs (the state after p items), the goal is x_p.
// Positions beyond T are not evaluated.  Built like UserSplit, from the user's two offsets, the engine's T and the call's min_history.
struct UserPrefix {
    int L, fed, first;
    __host__ __device__ constexpr UserPrefix(long long off_lo, long long off_hi, int T, int min_history)
        : L((int)(off_hi - off_lo)), fed(L < 1 ? 0 : (L - 1 < T ? L - 1 : T)), first(min_history) {}
    __host__ __device__ constexpr int n_pos() const { return fed >= first ? fed - first + 1 : 0; }
    __host__ __device__ constexpr int first_pos() const { return first; }
    __host__ __device__ constexpr int last_pos() const { return fed; }
    __host__ __device__ constexpr int place(int p) const { return p - first; }      // of position p among the user's results
};
#define SBR_PREFIX_IS(L, T, M, FED, NP) (UserPrefix(100, 100 + (L), (T), (M)).fed == (FED) && UserPrefix(100, 100 + (L), (T), (M)).n_pos() == (NP))
// (L, T, min_history) -> items fed, positions; L - 1 shorter than, equal to and longer than T
static_assert(SBR_PREFIX_IS(2, 6, 1, 1, 1) && SBR_PREFIX_IS(2, 6, 2, 1, 0) && SBR_PREFIX_IS(1, 6, 1, 0, 0), "L = 2: one item fed, one position; L = 1: none");
static_assert(SBR_PREFIX_IS(5, 6, 1, 4, 4) && SBR_PREFIX_IS(7, 6, 1, 6, 6) && SBR_PREFIX_IS(8, 6, 1, 6, 6) && SBR_PREFIX_IS(40, 6, 1, 6, 6), "never more than T items fed");
static_assert(SBR_PREFIX_IS(4, 6, 3, 3, 1) && SBR_PREFIX_IS(3, 6, 3, 2, 0) && SBR_PREFIX_IS(40, 6, 3, 6, 4), "positions start at min_history");
static_assert(UserPrefix(100, 140, 6, 3).place(3) == 0 && UserPrefix(100, 140, 6, 3).place(6) == 3, "results in order of p");
#undef SBR_PREFIX_IS

// The hashed draws of the batch builder (sbr_batch.hip) and of sbr_evaluate_candidates' negatives, stated for the device and the host
// alike: what a kernel draws, sbr_eval_negatives_host restates bit for bit.
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long x) {      // splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// Draw `si` of a sample set seeded by `seed`: uniform over the items, or the inverse of the CDF table.  The batch's negatives
// (bb_pack_kernel), the cluster head's own samples (bb_cluster_ids_kernel) and the evaluation's negatives follow this one law.
__host__ __device__ __forceinline__ int bb_draw_item(unsigned long long seed, int si, const double* __restrict__ cdf, int n_items) {
    const unsigned long long r = mix64(seed ^ mix64(0xA5A5ull + (unsigned long long)si));
    if (!cdf) return (int)(r % (unsigned long long)n_items);      // np.random.choice(n_items, S) (rnn_sampling.py:191)
    // bisect(cumsum, uniform(0, cumsum[-1])) (:159-163)
    const double x = (double)(r >> 11) * (1.0 / 9007199254740992.0) * cdf[n_items - 1];
    int lo = 0, hi = n_items;                                     // first index with cdf[idx] > x
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] > x) hi = mid; else lo = mid + 1; }
    return lo < n_items - 1 ? lo : n_items - 1;
}
// The negatives of user u in sbr_evaluate_candidates (include/sbr_rnn.h), the one statement of the rule: attempt
// t = 0, 1, .. draws bb_draw_item(ev_neg_seed(seed, u), t, neg_cdf, N); an attempt is accepted when its item occurs nowhere in the
// user's sequence and was not accepted before; the draw ends at n_negatives accepted or after ev_neg_attempts(n_negatives) attempts.
__host__ __device__ __forceinline__ unsigned long long ev_neg_seed(unsigned long long seed, int user) {
    return mix64(seed ^ mix64(0xCA4Dull + (unsigned long long)user));
}
__host__ __device__ constexpr int ev_neg_attempts(int n_negatives) { return 16 * n_negatives + 256; }
static_assert(ev_neg_attempts(250) == 4256 && ev_neg_attempts(299) == 5040, "the attempt cap of the draw");
constexpr int kEvCandSeqLds = 1024;       // ev_cand_build_kernel: longest sequence kept as a hash set in LDS (8 KB); above: searched in memory
constexpr int kEvCandThreads = 256;       // threads of a row's workgroup in ev_cand_build_kernel = attempts of the draw decided per round
// slots of the LDS hash set of the accepted negatives: a power of two with room for n_negatives + one round of attempts at 2/3 load
static inline int ev_neg_hash_slots(int n_negatives) {
    int slots = 64;
    while (slots < (n_negatives + kEvCandThreads) * 3 / 2) slots <<= 1;
    return slots;
}

// Every environment switch the library reads (README.md "Switches"), with its default.  sbr_read_switches (sbr_api.hip) fills one
// per engine, inside sbr_create, and nothing reads the environment afterwards: an engine keeps the values it was created under.
#define HEAD_WAIT_TICKS 6000ull      // 60 us of the 100 MHz clock: how long a chunk's statistics are waited for before they are recomputed
struct SbrSwitches {
    int rpt = 0;                 // SBR_RPT=1,2,4,8,16: rows per workgroup of the bf16x6 recurrent kernels (else: chosen by the batch size)
    int bwd_chunks = 1;          // SBR_BWD_CHUNKS: BPTT launches per layer (1..SBR_BWD_CHUNKS)
    int cluster = 1;             // SBR_CLUSTER: cluster recurrent kernels for wide layers
    int cl_linear = 0;           // SBR_CL_LINEAR: (experiment) cluster members on consecutive workgroup ids = different XCDs
    int cl16 = 1;                // SBR_CL16: the 16-row cluster kernels (sbr_rec_c16.hip); 0: the 8-row ones
    int c16_two_level = 1;       // SBR_C16_TWO_LEVEL: Hp = 512, the backward exchange in two levels (rec_bwd_c16t)
    int x6_pipe = 1;             // SBR_X6_PIPE: per-k-block publish counters instead of a workgroup barrier per step (0: the barrier kernels, x6s)
    int x6_f16 = 1;              // SBR_X6_F16: forward chains on the two-plane fp16 split (sbr_rec_f16_fwd)
    int x6_f16_bwd = 1;          // SBR_X6_F16_BWD: ... and the BPTT chains (sbr_rec_f16_bwd)
    int fuse_gather = 1;         // SBR_FUSE_GATHER: the embedding gather inside the forward kernel
    int gemm_f16 = 1;            // SBR_GEMM_F16: the dense GEMMs around the recurrent layers on the two-plane fp16 split
    int wgrad_f16 = 1;           // SBR_WGRAD_F16: ... and the dW_hid GEMM
    int tail_overlap = 1;        // SBR_TAIL_OVERLAP: weight-gradient GEMM and scatter-add of finished time chunks run beside the BPTT chain
                                 // (2: the same kernels on the main stream behind the chain)
    int tail_scatter_lds = 1;    // SBR_TAIL_SCATTER_LDS: its scatter-add in LDS rows; 0: the polling range form (also the way out when the LDS rows run out)
    int tail_trace = 0;          // SBR_TAIL_TRACE: the consumers' wait stamps (SbrPoll.trace, tools/tail_trace.py)
    int scat_range = 1;          // SBR_SCAT_RANGE: scatter-add of wide rows -- 1 the range form up to 1024-float rows, the atomic kernel beyond (C5:
                                 // measured 8.35 against 8.44 - 8.48 ms with either new form); 2 the segment-parallel form; 0 the atomic kernel everywhere
    int sparse_out_early = 1;    // SBR_SPARSE_OUT_EARLY: the sampled head's row-sparse block is caught up beside the forward chain and stepped
                                 // beside the BPTT chain (side stream) instead of in front of / behind them
    int head_fuse = 1;           // SBR_HEAD_FUSE: the full-softmax / sampled head in one launch (sbr_head.hip)
    unsigned long long head_wait_ticks = HEAD_WAIT_TICKS;   // SBR_HEAD_WAIT_TICKS (tests: 0 = every foreign chunk is recomputed)
    int out_fuse = 1;            // SBR_OUT_FUSE: the dense head's gradient and step in one launch (launch_out_grad_step)
    int row_aware = 1;           // SBR_ROW_AWARE_UPDATE: the dense pass over a wide index-input block skips the gradient traffic of the rows the batch did not touch
    int cluster_rank = 1;        // SBR_CLUSTER_RANK: sbr_cluster_rank scores only the members of each row's cluster (sbr_cluster_rank.hip); 0: it
                                 // gathers them from the full score matrix (also the road of the bf16 / triage projections)
    int cand_rank = 1;           // SBR_CAND_RANK: sbr_rank_candidates / sbr_evaluate_candidates score only each row's candidates (sbr_cand_rank.hip); 0: they gather them
                                 // from the full score matrix (also the road of the bf16 / triage projections)
};

// Which recurrent kernel serves a layer, and everything the step and sbr_query derive from that choice.  Every input of the
// decision is fixed when the engine is created, so sbr_rec_plan (sbr_rec.hip) makes it once per layer, inside sbr_create, and the
// launchers, the step and the queries read the answer: this is what makes the forward and the backward launch of a step agree on the
// layout of the saved activations they share.
enum RecKernel { REC_TRIAGE, REC_C16, REC_CL8, REC_X6P, REC_X6Q, REC_X6S, REC_X6, REC_MFMA };
struct RecPlan {
    RecKernel fwd, bwd;          // what launch_rec_forward / launch_rec_backward run
    int family;                  // sbr_query "rec_kernel": 0 triage, 1 cluster, 2 x6p, 3 x6q, 4 other
    int fwd_rows, bwd_rows, fwd_wgs, bwd_wgs, products_fwd, products_bwd;   // sbr_query "rec_rows_*" / "rec_workgroups_*" / "rec_products_*"
    int bwd_blocks;              // part[] blocks the backward launch writes
    bool bwd_chunkable;          // the backward launch honours RecArgs.t_lo / t_hi / chunk (bf16x6 kernels)
    bool fuse_gather;            // the forward launch gathers the rows of W_in itself: the step sets RecArgs.gX / gWin / gbias
    bool tail_ok;                // rec_bwd_x6p's progress-publishing form can serve the layer (overlapped step tail)
    bool needs_fill;             // cluster kernels: the backward exchange arrays want their sentinel fill (sbr_rec_bwd_cl_fill)
    size_t fwd_lds, bwd_lds; int bwd_dbuf;   // REC_X6S / REC_X6 / REC_MFMA: dynamic LDS of the launch, the backward's double buffer
};

// What means something only between the opening of a step (sbr_zero_grads) and its sbr_apply_update, or between an inference forward
// and its read-out; grouped by the phase that writes it.  step_reset (below sbr_handle) value-initialises all of it where a step can
// begin, so nothing of one step -- finished, failed or left half way -- reaches the next.
struct StepState {
    // sbr_zero_grads, sbr_forward
    bool step_open = false;      // sbr_zero_grads has opened a training step (cleared by sbr_forward)
    bool train_fwd_open = false;    // a training forward whose step has not reached sbr_apply_update
    int tail_nc = 0;                    // this step: tail_chunks for a training step, 0 (plain keys) for any other forward
    bool tail_sorted = false;    // this step: the sort already ran (sbr_forward)
    bool cells_early = false;    // this step: cells built + their rows caught up on the side stream by sbr_forward (ev_cells)
    bool fork_gated = false;              // this step: the second side stream was released by the start word (sbr_forward)
    unsigned marks_shared = 0;   // marks of this step already recorded as a cross-stream event (record_shared)
    // sbr_loss_backward_output
    bool fill_done = false;      // the cluster BPTT sentinel fill of this step was issued on the side stream (ev_fill)
    bool tail_gated = false;     // this step: the side stream is already behind a gate on this step's epoch (sbr_loss_backward_output)
    hipEvent_t ev_lg_rec = nullptr; // this step: the main-stream record that released the side stream (sbr_loss_backward_output); one of the handle's events (read by side_batch_work, in the same phase: sbr_build_batch reads the handle's ev_step_rec)
    int dh_slabs_n = 0;          // > 0: dh_last of this step sits in the main workspace as that many unreduced split-K slabs
    bool og_recorded = false;    // ev_og marks the output-layer gradients of this step complete
    // data-parallel exchange (sbr_sparse_pack*, sbr_sparse_unpack_add*)
    int sp_exchanged[2] = {0, 0}; // data-parallel step: rows of block b were packed / gathered (candidates = a_cand[0 .. sp_ncand[b]))
    int sp_ncand[2] = {0, 0};
    // Ranges of the parameter section that are already stepped, or whose step is already placed: written by the loss phase and
    // sbr_backward_recurrent, read by sbr_apply_update -- which, of the groups above, takes og_recorded and the exchange's lists only
    bool out_stepped = false;    // this step: done, the output layer's range needs no update launch
    bool out_early = false;      // this step's output-layer parameters were stepped on the side stream beside the BPTT chain
    bool wout_early = false;     // this step: the sampled head's rows were stepped beside the BPTT chain
    bool tail_updated = false;   // this step: the overlapped tail has applied the optimizer itself (single-call step)
    bool tail_swapped = false;   // this step: after the BPTT chain the main stream kept dW_hid, the side stream took the scatter (sbr_apply_update splits its ranges accordingly)
    bool rows_stepped[2] = {false, false};   // this step: block b's row step already ran in front of the join (update_sparse)
};

struct sbr_handle {
    Layout lay;
    SbrSwitches sw;
    ScatPlan scat;                           // layer 0's scatter-add (sbr_scat_plan, behind plan_layers and plan_tail)
    RecPlan plan[2 * SBR_MAX_LAYERS] = {};   // [l * D + d], like Layout.layer: filled by plan_layers at the end of sbr_create
    float* arena = nullptr; bool own_arena = false;
    hipStream_t stream = nullptr;
    // Priority side streams and disable-timing events: sbr_create / sbr_destroy walk handle_streams() / handle_events() (sbr_api.hip)
    hipStream_t side = nullptr;      // batch-only preprocessing (scatter sort) overlapped with the chain
    hipStream_t side2 = nullptr;     // second consumer stream of the overlapped tail (scatter-add)
    hipStream_t side3 = nullptr;     // the overlapped tail's monitor where it is a launch of its own (tail_monitor_kernel), and s_bb
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_sort = nullptr, ev_lg = nullptr, ev_fill = nullptr, ev_og = nullptr, ev_chunk[SBR_BWD_CHUNKS] = {};
    hipEvent_t ev_cells = nullptr, ev_tail = nullptr, ev_tail2 = nullptr, ev_bb = nullptr, ev_bbw = nullptr;
    StepState st;                // this step: see above; everything below outlives it
    // call scope and stream state that outlives the step: a step left half way is joined by whoever comes next (side_join)
    bool in_train_step = false;  // phases called from sbr_train_step (set and cleared by that call's own scope): the side stream joins only before the update
    bool side_pending = false;   // side-stream work issued and not yet joined by the main stream
    bool deferred_join = false;  // phases called one by one do not join the side stream (sbr_set_deferred_join)
    bool tail_join_pending = false; // overlapped tail of a phase-by-phase step: the main stream has not joined the consumer streams yet
    // epochs: each word they stamp must differ from what ANY earlier launch left, so they only ever advance
    unsigned head_epoch = 0; int cl_epoch = 0, sp_epoch = 0;   // the one-launch head's, the cluster exchange's, the pack epoch
    int prog_epoch = 0;          // epoch of the chain's progress words: advanced once per step by tail_next_epoch (sbr_step.hip)
    int join_epoch = 0, fork_epoch = 0;   // epochs of the completion words / the start word: advanced by step_next_epoch (sbr_step.hip), never 0
    // engine-constant: plans, switches and buffers made by sbr_create or on first use
    std::vector<ParamDesc> descs;
    int rpt = 16;                // rows per workgroup for the bf16x6 recurrent kernels (SbrSwitches.rpt, or chosen by the batch size)
    bool timing = false; unsigned timing_marks = 0;   // which of the SBR_N_PHASES event marks a step records (sbr_enable_timing)
    int tail_chunks = 0, tail_ch = 0;   // the overlapped tail as sbr_create planned it (plan_tail): time chunks of the sort's keys (0: not taken), steps per chunk
    SbrTChunks tail_bounds = {};        // ... and their bounds
    unsigned long long* tail_trace = nullptr;    // SbrSwitches.tail_trace: SbrPoll.trace
    int scnt_zero_n = 0;                                                  // leading counters of a_scnt known to be zero (launch_scatter_sort)
    std::vector<int> tail_slab_host; int* tail_slab_dev = nullptr; int tail_slab_key[2] = {0, 0};   // the table of the last plan
    // Words of the step boundary (kStepJoinGate / kStepForkGate): an allocation of its own, made and zeroed on first use and freed by
    // sbr_destroy; each word on a 128-byte line of its own.  [32]: completion word of the side stream, [96]: of the second side
    // stream, [128]: the forward chain's start word.
    int* step_words = nullptr;
    // the lagged cost report: read one call later
    float* lag_host = nullptr;   // pinned: [2] cost, [2] fault flag, [2] sequence number (sbr_train_step_lagged: lag_report_kernel)
    unsigned lag_seq[2] = {0, 0}, lag_counter = 0;
    int lag_slot = 0, lag_pending = -1;
    // current batch: the arena's own buffers, or (device-resident inputs covering all Bp rows) the caller's
    const int *bX = nullptr, *blen = nullptr, *btgt = nullptr, *bsmp = nullptr; const float* bpop = nullptr;
    int n_rows = 0;          // rows of the current batch (<= local_batch)
    bool have_batch = false, fwd_done = false;   // (fwd_done: ranking and evaluation read the hidden state long after the forward)
    int64_t step_count = 0;  // adam t
    bool grads_clean = false;    // the gradient section is all zero (fresh arena, or the update kernel cleared it)
    // The hand-over to sbr_build_batch beside the step in flight (sbr_batch.hip), read by a build AFTER the step's calls have returned: its
    // own stream, the set the current batch sits in, and what tells it that the set it is about to overwrite is no longer read
#ifndef SBR_BB_STREAM
#define SBR_BB_STREAM 0      // (probe builds: 1 = a stream of its own, 2 = ... at low priority)
#endif
    hipStream_t s_bb = nullptr;
    int bb_set = 0;             // arena set of the current batch (0: also what sbr_set_batch fills)
    uint64_t batch_seq = 0;     // sbr_forward calls so far
    uint64_t set_use[2] = {0, 0};   // batch_seq of the last forward that read set i
    uint64_t lg_seq = 0;        // batch_seq when ev_step_rec was last set (a main-stream record in the middle of a training step)
    bool bb_unread = false;     // the current batch was built and no forward has read it yet
    int bb_slow = 0;            // builds left that wait for all of the engine's streams (a step was abandoned: its side streams were not joined)
    int step_word_epoch = 0;     // != 0: the forward chain of the step in flight publishes this epoch in its start word (sbr_build_batch waits for it
                                 // where it waited for ev_step_rec)
    hipEvent_t ev_step_rec = nullptr; // a main-stream record made DURING the step in flight, for sbr_build_batch: StepState.ev_lg_rec, or the forward's fork
    // what the last call ran, for sbr_query: read at any time
    // sbr_rank: scratch outside the arena (grown on demand, freed by sbr_destroy) and what the last call ran (sbr_query "rank_select" / "rank_sort")
    void* rank_scratch = nullptr; size_t rank_scratch_bytes = 0; int last_rank_select = 0, last_rank_sort = 0;
    int last_goal_rank_form = 0;                                          // sbr_evaluate_ranks: 0 none yet, 1 the row's keys in LDS, 2 streamed
    int last_next_rank_form = 0;                                          // sbr_evaluate_positions: 0 none yet, 1 16-byte loads of the score row, 2 4-byte loads
    int last_logprob_form = 0;                                            // sbr_evaluate_logprob, _positions_logprob, sbr_debug_row_logprob: the same two forms
    int last_next_rank_slots = 0;                                         // ... and the positions it projected per GEMM launch at the most
    int last_cluster_rank_form = 0;                                       // sbr_cluster_rank: 0 none yet, 1 restricted scoring, 2 gathered from the full scores
    int last_replay_launches = 0;                                         // sbr_sessions_replay: the kernel launches the most recent one enqueued
    int last_park_chunks = 0;                                             // sbr_sessions_export / _import: the chunks the most recent one staged
    int last_replay_rank_passes = 0, last_event_rank_form = 0;            // sbr_sessions_replay_ranks: the passes (tracing replay launches) of the most recent call; its count's loads as last_next_rank_form
    int last_cand_rank_form = 0;                                          // sbr_rank_candidates / sbr_sessions_rank_candidates: 0 none yet, 1 only the candidates scored, 2 gathered from the full scores
    int last_eval_cand_form = 0, last_eval_cand_lmax = 0;                 // sbr_evaluate_candidates: the same two forms (0 none yet); the width of the last chunk's compact score matrix
    int last_tail_gated = -1;                                             // ... sbr_query "tail_gate_first"
    int last_scatter_form = -1; bool last_row_aware = false;              // what the last step launched: sbr_query "scatter_form" / "row_aware_update"
    int last_join_gate = -1, last_fork_gate = -1;                         // what the last step took: sbr_query "step_join_gate" / "step_fork_gate"
    // ring of per-step event sets, read back after the timed region (no per-step sync)
    static const int kRing = 64;
    hipEvent_t ev[kRing][SBR_N_PHASES] = {};
    int ring_used = 0;       // train steps recorded since timing was enabled
    int ring_cur = 0;        // set used by the step in flight
    // chain-only timing (sbr_chain_times): an event pair around every launch of a recurrent chain kernel, any layer, either direction
    static const int kChain = 256;
    hipEvent_t ev_ch[kChain][2] = {};
    unsigned char ch_dir[kChain] = {};
    int ch_n = 0;
    bool chain_timing = false;
    float* P(size_t off) const { return arena + lay.s_params + off; }
    float* Gd(size_t off) const { return arena + lay.s_grads + off; }
    float* St(int k, size_t off) const { return arena + lay.s_state + (size_t)k * lay.n_params + off; }
    float* A(size_t off) const { return arena + lay.s_act + off; }
    float* cost_ptr() const { return arena + lay.s_grads + lay.n_params; }
};
// A training forward still open where a step begins (step_reset) or a batch is built (sbr_build_batch) will not reach its
// sbr_apply_update, or has not yet: its side streams are not joined, so the next two batch builds wait for every stream.
static inline void step_abandoned_check(sbr_handle* h) { if (h->st.train_fwd_open) h->bb_slow = 2; }
// The one reset of the per-step state, which looks before it clears.  Called where a step can begin, ends or is discarded: sbr_zero_grads,
// sbr_forward when no step is open (predict, top-k, rank, evaluate), the end of sbr_apply_update, sbr_state_load.
static inline void step_reset(sbr_handle* h) { step_abandoned_check(h); h->st = StepState{}; }

// The cluster head (sbr_cluster.hip; include/sbr_rnn.h "The cluster head of RNNCluster")
struct sbr_cluster {
    sbr_cluster_config cfg;
    hipStream_t stream;
    float *R, *Wc, *dR, *dWc, *sR[2], *sWc[2];       // parameters, gradients, optimizer state
    float *z, *p, *M, *sm, *sg, *score, *dz, *rowcost, *ones, *cost, *hard, *nused;
    int* ids;
    long step;
    float scale;
    unsigned long long noise_ctr;
    int J;                                           // cells of the last forward (B + samples)
    int hard_valid;
    // sbr_cluster_evaluate's PRODUCT road (sbr_cluster_eval.hip): the same floats as `hard`, [C][N], so that a row's membership column
    // is a contiguous stream.  Own allocation, made on first use; valid only while hard_valid is (every site that clears one clears both)
    float* hardT; int hardT_valid;
    int dR_clean;                                    // dR is all zeros: the optimizer kernel clears every gradient it consumes (no N x C memset per step)
    // sbr_cluster_lists / sbr_cluster_rank (sbr_cluster_rank.hip): the hard clusters of prepare_tests as a CSR over clusters.  Own
    // allocations, made on first use and freed by sbr_cluster_destroy; valid until R changes (set_params, apply_update)
    int lists_valid;
    int* mem_ids; size_t mem_cap;                    // [sum of sizes] item ids, every list ascending
    int* mem_off;                                    // [C + 1] first entry of every list
    int* mem_work; size_t mem_work_n;                // [C][blocks] per-block counts, then exclusive offsets inside a list
    std::vector<int> mem_sizes;                      // host copy of the sizes, read back once per version of R
    int lmax;                                        // the longest list, padded to a multiple of 4
};

// The session pool (sbr_session.hip; include/sbr_rnn.h "Stateful sessions").  Own allocations, freed by
// sbr_sessions_destroy.  A slot's state in layer l is row `slot` of plane (events[slot] & 1) of hs[l] / cs[l]: a step reads that plane
// and writes the other, and the commit launch at the end of sbr_sessions_advance makes the written one current by counting the event.
struct SesPool {                                     // what the kernels read: passed by value
    long long capacity; int L, ring_len, history;
    int Hp[SBR_MAX_LAYERS];
    float* hs[SBR_MAX_LAYERS];                       // [2][capacity][Hp]
    float* cs[SBR_MAX_LAYERS];                       // [2][capacity][Hp], LSTM only (else NULL)
    long long* events;                               // [capacity] events fed
    int* ring;                                       // [capacity][ring_len]: the id of event e at e % ring_len (ring_len = max(history, 1))
};
// A parked session (include/sbr_rnn.h "The record of a parked session"): int64 events, int32 ids[ring_len]
// oldest first then -1, zeros up to `head` (a multiple of 16 bytes), then per layer h[Hp] (and c[Hp], LSTM) of the CURRENT plane
struct SesRecLayout { size_t bytes, head; int L, ring_len, lstm; int Hp[SBR_MAX_LAYERS]; };
struct SesRow { long long start, len; int slot; };   // a row of sbr_sessions_replay: items[start .. start + len) go to slot
// beside a SesRow of a tracing pass (sbr_sessions_replay_ranks): the state before its event t goes to row at + t of the pass's trace;
// first: where the row's list starts in the call's events (event t of the pass is event start + t - first of the call); call_row:
// the row of the call, which names the event count and ring kept aside
struct SesTraceRow { long long at, first; int call_row; };
struct sbr_sessions {
    sbr_handle* h;
    SesPool p;
    int *d_slots, *d_items, *d_second;               // [capacity] each: the lists of the call in flight (slots of a call are distinct)
    // sbr_sessions_replay: its rows ([capacity], allocated by the first replay) and the events of the call in flight ([ev_cap] each,
    // grown when a call needs more and kept); rows: the host's copy, longest first
    SesRow* d_rows; int *d_ev_items, *d_ev_second; long long ev_cap;
    std::vector<SesRow> rows;
    std::vector<unsigned> stamp; unsigned epoch;     // host: stamp[slot] == epoch: the slot was already named in this call
    // sbr_sessions_export / _import: the record layout of this pool and the staging buffer of the chunk in flight (park_cap bytes:
    // the chunk's records, then its slot list; grown when a call needs more and kept)
    SesRecLayout rec; unsigned char* d_park; size_t park_cap;
    std::vector<int> park_ids;                       // host: the ids of the record import is checking
};
// sbr_session.hip: the kernels behind the calls.  Every slot, id and row count was checked on the host
hipError_t launch_ses_reset(hipStream_t s, const SesPool& p, const sbr_handle* h, const int* slots, long long n);
hipError_t launch_ses_gather_top(hipStream_t s, const SesPool& p, const int* slots, int rows, float* out);      // out [rows][Hp of the top layer]
// ... and the two checks every sessions call starts with: no training step open and no lagged cost pending (SBR_ESTATE); the slots
// inside the pool and, with distinct, named once (SBR_EINVAL)
int sessions_state_check(const sbr_sessions* s, const char* call);
int sessions_check_slots(sbr_sessions* s, const char* call, const int32_t* slots, long long n, bool distinct);
// ... and the pieces of sbr_sessions_replay that sbr_sessions_replay_ranks (sbr_rank_api.hip) runs as well: what is refused about the
// lists, the device copy of the events (the pool's d_ev_items / d_ev_second; flushes the lazily stepped index-input rows), one replay
// launch over device rows (trace != NULL: the tracing form), and the event counts [n] and rings [n][ring_len] (NULL: not) of the
// call's slots kept aside
int ses_replay_check(sbr_sessions* s, const char* call, const int32_t* slots, int64_t n, const int32_t* items, const int32_t* second,
                     const int64_t* off);
int ses_replay_events(sbr_sessions* s, const char* call, const int32_t* items, const int32_t* second, int64_t total);
hipError_t launch_ses_replay_rows(sbr_sessions* s, const SesRow* d_rows, int n_rows, bool second, const SesTraceRow* trows, float* trace);
hipError_t launch_ses_keep(hipStream_t st, const SesPool& p, const int* slots, long long n, long long* e0, int* ring);
// sbr_eval.hip: one workgroup per row of a group of traced states, g0 the group's first trace row; scores [rows][N] are written (-inf
// at the excluded ids) and then counted
struct SesEventRank {
    const SesRow* rows; const SesTraceRow* trows; int n_rows;      // the pass
    const int* items; const long long* keep_e0; const int* keep_ring; int ring_len, history, mode;
    long long g0; float* scores; int N; int *ranks, *n_rankable;
};
hipError_t launch_ses_event_rank(hipStream_t s, const SesEventRank& a, int rows, int* form);

void sbr_set_error(const char* fmt, ...);
#define SBR_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    sbr_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return SBR_EHIP; } } while (0)

#define CHECK_ARG(cond, ...) do { if (!(cond)) { sbr_set_error(__VA_ARGS__); return SBR_EINVAL; } } while (0)
#define SBR_LAUNCH(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    sbr_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return SBR_EHIP; } } while (0)

// What the ranking and evaluation calls (sbr_rank_api.hip) need of the engine (sbr_api.hip, sbr_step.hip)
int flush_lazy(sbr_handle* h, int only_kind = -1);   // every row of every sparse block (of that kind) current through the last applied step
bool simple_gemm(const sbr_handle* h);               // SBR_FLAG_SIMPLE_GEMM: the triage projection
float* h_last(sbr_handle* h);                        // the user representation of the current batch, [Bp][HLt]
int check_fault(sbr_handle* h);                      // synchronises the stream; fails the call if a bounded wait of its kernels gave up
int full_scores(sbr_handle* h, int do_softmax);      // forward_current + the projection into a_logits: the scores of every item
int project_rows(sbr_handle* h, const float* rows_in, int n_rows, float* out, int do_softmax);   // full_scores' launch pair on any [n_rows][HLt] matrix of states
int forward_current(sbr_handle* h);                  // (sbr_rank_api.hip) forward pass if the batch has none yet + lazily stepped output rows flushed
// What the cluster head's native training step (sbr_cluster.hip: sbr_cluster_train_step_lagged) needs of its neighbours
struct sbr_dataset;
int cluster_fits_engine(const sbr_cluster* c, const sbr_handle* h);      // (sbr_rank_api.hip) items, width and split of the user representation, stream
int dataset_fits_engine(const sbr_dataset* d, const sbr_handle* h);      // (sbr_batch.hip) items, stream
// (sbr_batch.hip) ids [n_tgt + n] = targets ++ (samples given: its first n entries; NULL: n draws by d's sampling law from `seed`), one launch
hipError_t launch_cluster_ids(hipStream_t s, const sbr_dataset* d, const int* targets, int n_tgt, const int* samples, int n,
                              unsigned long long seed, int* ids);

// What the rest of the engine (sbr_api.hip: sbr_query, sbr_zero_grads, the sparse exchange, the debug calls) needs of the training
// step (sbr_step.hip), and the one layout piece the step takes from there
struct RecArgs; struct SbrSparseRows; struct SbrSparseUpd;
void plan_layers(sbr_handle* h);                     // fills h->plan from the layout, the switches and the flags (sbr_create, once)
void plan_tail(sbr_handle* h);                       // overlapped step tail: fills h->tail_chunks / tail_ch / tail_bounds (sbr_create, once, behind plan_layers)
bool head_sampled_taken(const sbr_handle* h, int rows);   // does a step over `rows` rows take the one-launch sampled head?
void mark(sbr_handle* h, int i);                     // timing mark i of the step in flight, on the main stream
SbrSparseRows sparse_rows(sbr_handle* h, int b);     // row-sparse block b: where its rows, gradients, state and last-step words are
SbrSparseUpd sparse_upd(sbr_handle* h);              // ... and the optimizer's constants for the row kernels
// ... and the ids its own step walks (list, n_dev, n_host, n_max of the launch_sparse_* list kernels).  kind 0: the plain-key sort's
// ids, counted on the device by the sort's last offset; kind 1: the C sampled cells
struct SbrSparseIds { const int* list; const int* n_dev; int n_host, n_max; };
SbrSparseIds sparse_ids(const sbr_handle* h, int b);
int side_join(sbr_handle* h);                        // the main stream joins whatever the step left pending on the side streams
// adagrad's zero-gradient step is a no-op: nothing is ever pending
static inline bool sparse_lazy(const sbr_handle* h) { return h->lay.n_sparse > 0 && h->lay.cfg.updater != SBR_UPD_ADAGRAD; }
// one direction's counting-sort arrays of the batch's ids (dir 0: a_s*, 1: the reversed ids of --r_bi, a_s2*): counters, segment
// offsets (off[n_ids]: the entry count), cursors, and the sorted entries' ids and positions
struct SbrSortKeys { int *cnt, *off, *cur, *sid, *pos; };
SbrSortKeys sort_keys(const sbr_handle* h, int dir);
// (sbr_api.hip) the float ranges of the parameter section that the row-sparse blocks own, ascending
std::vector<std::pair<size_t, size_t>> sparse_float_ranges(const Layout& lay);

// Consumers of a RUNNING BPTT chain (overlapped step tail): the chain's waves publish (epoch << 12) | t in words[0 .. n) once
// all their time steps >= t are complete and written through (RecArgs.progress); ONE workgroup -- the MONITOR: workgroup 0 of
// the scatter-add launch, or tail_monitor_kernel -- folds them into `done` = (epoch << 12) | max t, which every consumer polls.  rows_per_step: K rows per time step.
// Slabs of a polling GEMM are K-ascending, slab z = rows [slab_lo[z], slab_lo[z + 1]) (a device table of multiples of 32, see
// sbr_tail_slab_table: one k step of 32 rows for the time steps the chain reaches last, growing with the time the chain still
// needs once a slab is released -- a slab must be DONE when the chain ends, not started); workgroups take them from the far end.
// The monitor's word exists in SBR_DONE_COPIES copies, SBR_DONE_STRIDE ints apart (4 KB + 256 B: other pages AND other channels):
// hundreds of waves poll it with agent-scope loads, which are served by the memory side, and each poller reads the copy its
// workgroup number selects.  (Built on the suspicion that ONE word makes every poll queue at one channel; the consumers' slow
// loads of profiles/round3_n_trace.txt turned out to have other causes -- DESIGN.md 3a -- and the copies cost nothing.)
// Dynamic LDS above the default limit needs the function attribute -- once per kernel and size, not per launch (a driver call
// each: six of them per training step before round 3c, on a path whose host side is as long as its device side).  One static
// per expansion site, i.e. per kernel; one process drives one GPU.
#define SBR_DYN_LDS(KERNEL, LDS) do { static int sbr_dyn_lds_set_ = -1; if ((int)(LDS) > sbr_dyn_lds_set_) { \
        (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS)); sbr_dyn_lds_set_ = (int)(LDS); } } while (0)
#define SBR_DONE_COPIES 32
#define SBR_DONE_STRIDE 1088
struct SbrPoll { const int* words; int n; int* done; int epoch; int rows_per_step; int* fault; int n_small, k_small;
                 unsigned long long* trace; const int* slab_lo; int n_slabs; };    // trace (sbr_handle.tail_trace, tools/tail_trace.py): 100 MHz stamps of the consumers' waits and ends

// ---------------------------------------------------------------------------------------
// Kernel launchers (each returns hipGetLastError())
// ---------------------------------------------------------------------------------------
// K1: xt[t][b][:] = sum_f W_in[X[b][t][f]][:] + bias         (sparse_lstm.py:368,:755,:1111)
hipError_t launch_gather_xt(hipStream_t s, const float* Win, const float* bias, const int* X, float* xt,
                            int T, int Bp, int F, int GHp, int n_rows_in);
// K6: dWin[X[b][t][f]][:] += dxt[t][b][:] for t < len[b]     (AdvancedIncSubtensor grad [3P])
hipError_t launch_scatter_rows(hipStream_t s, float* dWin, const float* dxt, const int* X, const int* len,
                               int T, int Bp, int F, int GHp);
// counting sort of the valid (position, id) pairs by id (depends on the batch only), then one wave per
// chunk of 32 sorted entries reduces the dxt rows of equal id in registers
// concat != 0: entry (pos, f) addresses row pos*F + f of the gradient array (embedding layer: the F embeddings of a step are
// concatenated, not summed)
// tch > 0: time-chunked keys chunk(t) * n_ids + id over the n_tchunks chunks of *bounds (cnt / offs / cur then hold n_tchunks * n_ids + 1 ints)
hipError_t launch_scatter_sort(hipStream_t s, const int* X, const int* len, int T, int Bp, int F, int n_ids, int* cnt,
                               int* offs, int* cur, int* sid, int* spos, int concat = 0, int tch = 0, int n_tchunks = 1, const SbrTChunks* bounds = nullptr,
                               int* cnt_zero_n = nullptr);
int sbr_scatter_lds_ids();     // largest key space the LDS-histogram sort takes
// overlapped step tail: wait (bounded) until every progress word of the running BPTT chain is (epoch, <= target)
hipError_t launch_tail_gate(hipStream_t s, const int* progress, int n, int epoch, int target, int* fault);
// ... the same wait as ONE wave that may be launched long before the chain (it sits beside the forward chain and the head)
hipError_t launch_tail_gate_wave(hipStream_t s, const int* progress, int n, int epoch, int target, int* fault);
// step boundary: ONE wave waits (bounded: SBR_POLL_TICKS, fault bit 3) until w0[0] == epoch and, where w1 is given, w1[0] == epoch
hipError_t launch_step_gate(hipStream_t s, const int* w0, const int* w1, int epoch, int* fault);
// ... and what it waits for at the end of a stream: a one-lane kernel that stores `epoch` into `word` at its entry, i.e. once
// everything in front of it on stream s is complete and written back
hipError_t launch_step_word(hipStream_t s, int* word, int epoch);
// emb[t][b][f*Ep + e] = W_emb[X[b][t][f]][e]          (lasagne EmbeddingLayer + flatten(outdim=3), recurrent_layers.py:48)
hipError_t launch_gather_concat(hipStream_t s, const float* Wemb, const int* X, float* out, int T, int Bp, int F, int Ep);
// --r_bi helpers (sbr_misc.hip).  rev(t, len) = t < len ? len-1-t : t (padding stays in place).
hipError_t launch_rev_rows_int(hipStream_t s, const int* X, const int* len, int* Xr, int T, int Bp, int F);
hipError_t launch_rev_rows(hipStream_t s, const float* src, const int* len, float* dst, int T, int Bp, int W);   // dst[t][b] = src[rev(t)][b]
// cat[t][b] = [hs_f[t+1][b] | hs_b[rev(t)+1][b]]   (hs_*: [T+1][Bp][Hp], slot t+1 = state after step t of that scan)
hipError_t launch_cat_outputs(hipStream_t s, const float* hs_f, const float* hs_b, const int* len, float* cat, int T, int Bp, int Hp);
hipError_t launch_hcat(hipStream_t s, const float* hf, const float* hb, float* out, int Bp, int Hp);            // [hf | hb]
hipError_t launch_split_cols(hipStream_t s, const float* src, float* a, float* b, int rows, int Hp);             // src [rows][2Hp] -> a, b
// d[t][b] = f[t][b] + r[rev(t)][b] over W columns; then out_f[t][b] = d[t][b][0:Hp], out_b[t][b] = d[rev(t)][b][Hp:2Hp]
// (out_b == NULL: W arbitrary, only the sum d is written to out_f -- the embedding case)
hipError_t launch_uncat(hipStream_t s, const float* f, const float* r, const int* len, float* out_f, float* out_b, int T, int Bp,
                        int W, int Hp);
// The scatter-add of the sorted entries (sbr_scatter.hip): the launchers take the form's recipe from the engine's ScatPlan as given.
// form 1, wide rows (512 .. 1024 floats): range scatter-add, two passes, no atomics
hipError_t launch_scatter_range(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs, int n_ids,
                                int GHp, float* part, int* part_id, int n_ranges, const ScatPlan& plan);
#define SBR_SCAT_RANGES 512
// form 2 (512 .. 2048 floats): segment-parallel scatter-add, no atomics on rows
hipError_t launch_scatter_wide(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs, int n_ids,
                               int max_entries, int GHp, float* part, int* aux, int n_slots, const ScatPlan& plan);
// form 0: one wave per 32 sorted entries sums the rows of equal id in registers
hipError_t launch_scatter_reduce(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos,
                                 const int* offs, int n_ids, int max_entries, int GHp, int Bp, const ScatReduce& recipe);
// form 4: all time chunks of a time-chunked sort in ONE launch beside the running chain: every wave waits for poll.done to reach the
// time chunk of its entries, rows are added with float atomics (an id may occur in every chunk)
hipError_t launch_scatter_reduce_poll(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs,
                                      int n_ids, int n_tchunks, int max_entries, int GHp, int Bp, const SbrPoll& poll,
                                      const SbrTChunks& bounds, int short_chunks, bool fence_on, const ScatPlan& plan);
// form 5: the same without a global atomic per piece: `units` workgroups own id ranges of equal cost (P: n_ids + 1 ints of workspace,
// the running cost, which launch_scatter_cost_scan leaves behind the time-chunked sort) and accumulate their rows in LDS
hipError_t launch_scatter_cost_scan(hipStream_t s, const int* offs, int* P, int n_ids, int n_tchunks, const ScatPlan& plan);
hipError_t launch_scatter_lds_poll(hipStream_t s, float* dWin, const float* dxt, const int* sid, const int* spos, const int* offs, const int* P,
                                   int n_ids, int n_tchunks, int GHp, const SbrPoll& poll, const SbrTChunks& bounds,
                                   int units, const ScatPlan& plan, bool monitor = false, int t_lo = 0);      // monitor: one more workgroup, the tail's monitor
hipError_t launch_tail_monitor(hipStream_t s, const SbrPoll& poll, int t_lo);

// Tile-blocked activation layout [t][row tile of 16][column tile of 16][row 16][col 16] (floats):
// the 16x16 tile one wave of the recurrent kernels owns is one contiguous KiB (8 full 128-B lines per
// wave-wide 16-B access instead of 16 half lines of 16 different rows).  Used for xt (layer 0), the
// saved gate activations, dxt and dhi; hs/cs stay row-major for the GEMM consumers.
__host__ __device__ __forceinline__ size_t sbr_blocked_index(int t, int row, int col, int Bp, int ncols) {
    return (((size_t)t * (Bp >> 4) + (row >> 4)) * (ncols >> 4) + (col >> 4)) * 256 + (row & 15) * 16 + (col & 15);
}

struct RecArgs {
    int cell, T, Bp, H, Hp, G;
    float clip;
    const int* len;         // [Bp]
    const float* xt;        // [T][Bp][G*Hp]
    const float* Whid;      // [Hp][G*Hp]
    const float* peep;      // [3][Hp]
    const float* cinit;     // [Hp]
    const float* hinit;     // [Hp]
    float* hs; float* cs; float* g[4];
    // backward only
    const float* dh_last;   // [Bp][Hp] grad wrt the final hidden state (top layer) or NULL
    const float* dh_slabs;  // rec_bwd_x6p only: dh_last as n_dh_slabs unreduced split-K slabs of [Bp][Hp] (the kernel's prologue
    int n_dh_slabs;         // adds them: one small reduction launch less in front of the BPTT chain), or NULL / 0
    const float* dh_ext;    // [T][Bp][Hp] grad wrt every hid_out[t] (lower layers) or NULL
    int dhe_on;             // rec_bwd_c16 only (set by its launcher): dh_ext is live (else it points at hs and is only requested)
    float* dxt; float* dhi; // dhi: GRU only, compact [T][Bp][Hp] = candidate-gate slice of grad wrt hid_input (r,u slices == dxt)
    // BPTT in time chunks (so the weight-gradient GEMM of finished chunks runs beside the chain): this launch
    // covers t in [t_lo, t_hi); dh/dc cross launches through `state` [2][Bp][Hp]; part block = chunk*nblocks + block
    int t_lo, t_hi, chunk;
    float* state;
    float* part;            // [chunks][nblk][G*Hp + 5*Hp]
    int rpt;                // live batch rows per workgroup of the bf16x6 kernels (16, 8, 4, 2, 1); part[] has Bp/rpt blocks
    int xt_blocked;         // xt is tile-blocked (layer 0: written by the gather) or row-major (GEMM output)
    int x6_pipe;            // Hp = 128: waves synchronise per k-block through LDS counters, no per-step barrier (SbrSwitches.x6_pipe)
    int x6_f16, x6_f16_bwd; // fp16 planes allowed for the forward / the BPTT chain (SbrSwitches; what a launch takes: sbr_rec_f16_fwd / _bwd)
    int cl16, c16_two_level; // the 16-row cluster kernels allowed / their two-level backward exchange at Hp = 512 (SbrSwitches)
    // layer 0, one index per step: the embedding gather is fused into the forward kernel (xt is never written)
    const int* gX;          // [Bp][T] item ids, or NULL: read xt
    const float* gWin;      // [input_size][G*Hp]
    int n_in;               // rows of W_in (the pipelined kernels address them with 32-bit byte offsets)
    const float* gbias;     // [G*Hp]
    int f32_mfma;           // SBR_FLAG_F32_MFMA: exact-f32 v_mfma_f32_16x16x4_f32 kernels instead of bf16x6
    unsigned long long* prof; // SBR_FLAG_PROFILE_REC: [nblk][waves][4] cycle counters, else NULL
    // cluster kernels (sbr_rec_cl.hip): several workgroups per row tile for layers too wide for one CU
    int cluster;            // allowed (SbrSwitches.cluster)
    int cl_linear;          // (experiment, SbrSwitches.cl_linear) cluster members on consecutive workgroup ids = different XCDs
    int* fault;             // set to 1 when a cluster exchange wait gave up (bounded spin)
    int sentinel_done;      // the backward exchange arrays were already filled with the sentinel (side stream)
    int* clx;               // [tiles][C] start-of-launch handshake: (epoch << 4) | XCC id of every member
    void* xh;               // 16-row cluster kernels: ring [4][Bp/16][2 planes][16][Hp] fp16, the pre-split h exchange
    float* pring;           // ... and the ring of partial-sum blocks of the backward (sbr_rec_c16_ring_floats)
    int epoch;              // unique per launch (clx is never cleared)
    int relu;               // Vanilla layers with dense input = stock lasagne RecurrentLayer: rectify instead of tanh (sbr_cell.h)
    // overlapped step tail (rec_bwd_x6p only): dxt / dhi are stored write-through and every wave publishes
    // (prog_epoch << 12) | t in progress[block * 8 + wave] once all its time steps >= t are complete: at launch (t = first
    // live step + 1 ...), whenever t is a multiple of prog_every, and t_lo at the end.  NULL: plain stores, no progress
    int* progress; int prog_every; int prog_epoch;
    // step boundary (rec_fwd_x6p only): one lane of workgroup 0 stores start_epoch here at kernel entry, write-through -- whoever polls it
    // learns that everything in front of this launch on its stream is complete and written back.  NULL: nothing is stored
    int* start_word; int start_epoch;
    int fence_kb;           // rec_*_x6p: the workgroup claims this much of its CU's LDS (KiB; 0: what it needs) so that kernels which
                            // run BESIDE the chain and use LDS themselves are placed on other CUs (overlapped step tail)
};
// Operand planes of the recurrent chains (128-unit, small-layer and cluster kernels alike): the two-plane fp16 split unless it is
// switched off or its operand is unbounded -- forward: a rectified state (the split needs |h| < 65504); backward: the operand that
// carries gradients is bounded by the reference's own gradient clip at +-100.  Both values come from the engine's SbrSwitches.
static inline bool sbr_rec_f16_fwd(const RecArgs& a) { return a.x6_f16 && !a.relu; }
static inline bool sbr_rec_f16_bwd(const RecArgs& a) { return a.x6_f16_bwd && a.clip > 0.0f && a.clip <= 100.0f; }
#define SBR_CL_ROWS 8       // batch rows per cluster tile
#define SBR_C16_RING 2      // rec_bwd_c16: slots of the ring of partial-sum blocks (blocks carry the lap's parity: sbr_rec_c16.hip)
#define SBR_X6P_FUSE_MAX_T 4096      // fused gather of rec_fwd_x6p: 4 rows x T row offsets in LDS
// The plan of a layer: `shape` = its RecArgs without the batch (gX null; dh_ext set where a layer above feeds it), simple =
// SBR_FLAG_SIMPLE_REC, fused = the step would have the forward kernel gather W_in's rows (index input of one id per step, level 0,
// SbrSwitches.fuse_gather).  Pure host code: no handle, no HIP call.  The only caller of the per-family predicates below, which
// stay in the files that own their constants.
RecPlan sbr_rec_plan(const RecArgs& shape, bool simple, bool fused);
bool sbr_rec_cluster_ok(const RecArgs& a);    // sbr_rec_cl.hip: several workgroups per row tile, Hp = 256 / 512
bool sbr_rec_c16_ok(const RecArgs& a);        // ... on 16-row tiles (sbr_rec_c16.hip)
bool sbr_rec_x6p_ok(const RecArgs& a);        // sbr_rec_p.hip: pipelined bf16x6 kernels for Hp = 128 on 4-row tiles
bool sbr_rec_x6p_fuse_ok(const RecArgs& a);   // ... and its forward kernel can gather the W_in rows itself (never part of sbr_rec_x6p_ok)
bool sbr_rec_x6p_tail_ok(const RecArgs& a);   // ... and its backward kernel can publish progress (RecArgs.progress)
int sbr_rec_x6p_f16_terms();                  // MFMAs per f32 product of the x6p kernels' fp16 forms (2: packed planes, sbr_rec_p.hip)
bool sbr_rec_x6q_ok(const RecArgs& a);        // sbr_rec_q.hip: the same step loop for Hp = 32 / 64 (one wave per SIMD)
// The launches: the plan's kernel, taken as given.  The family launchers behind them (sbr_rec_cl.hip, sbr_rec_p.hip, sbr_rec_q.hip)
// refuse only what their kernels cannot run (hipErrorInvalidValue).
hipError_t launch_rec_forward(hipStream_t s, const RecArgs& a, const RecPlan& p);
hipError_t launch_rec_backward(hipStream_t s, const RecArgs& a, const RecPlan& p);
hipError_t launch_rec_forward_cl(hipStream_t s, const RecArgs& a, bool c16);
hipError_t launch_rec_backward_cl(hipStream_t s, const RecArgs& a, bool c16);      // (fills the exchange arrays first unless a.sentinel_done)
hipError_t sbr_rec_bwd_cl_fill(hipStream_t s, const RecArgs& a, bool c16);         // the sentinel fill of the backward exchange arrays
hipError_t launch_rec_forward_x6p(hipStream_t s, const RecArgs& a);
hipError_t launch_rec_backward_x6p(hipStream_t s, const RecArgs& a);
hipError_t launch_rec_forward_x6q(hipStream_t s, const RecArgs& a);
hipError_t launch_rec_backward_x6q(hipStream_t s, const RecArgs& a);
size_t sbr_rec_c16_ring_floats(int Bp, int Hp);
// sums the per-workgroup partials into bias / peephole / init gradients
hipError_t launch_rec_reduce_partials(hipStream_t s, const float* part, int nblk, int G, int Hp, int cell,
                                      float* db, float* dpeep, float* dcinit, float* dhinit);

// The dense GEMM:  C[m][n] = sum_k A(m,k) * B(k,n) (+ bias[n]), C row-major with leading dim ldc.
// How it runs is a value the caller passes (the engine builds its own from its flags in one place: sbr_step.hip); no launcher
// keeps a mode between calls.
struct GemmMode {
    bool simple = false;      // the triage kernel, one thread per output element (SBR_FLAG_SIMPLE_GEMM)
    bool exact_f32 = false;   // stay on the v_mfma_f32_16x16x4_f32 kernel, bitwise an fmaf chain (SBR_FLAG_F32_MFMA; scoring)
    // Operand planes of the tiled kernel (gemm_x6_kernel NP).  0: not stated, which means bf16x6.  1: plain bf16 operands, split-K
    // allowed (the layer GEMMs under SBR_FLAG_BF16_LAYERS).  2: the two-plane fp16 split (three MFMAs per product instead of
    // bf16x6's six) for operands the caller knows to be bounded: hidden states behind tanh / sigmoid gates, weights, gradients that
    // have passed the clip at +-100, with sa / sb the power-of-two scales that bring A / B into fp16's range.  3: bf16x6, stated.
    int planes = 0;
    float sa = 1.0f, sb = 1.0f;
    bool no_wide = false;     // stay on the 128-wide tile where the 256 x 128 one would be taken (parity tests of gemm_x6w_kernel)
    // Plain bf16 operands in ONE pass over K in a fixed order (no split-K), for any number of rows, so that an output element never
    // depends on M: the projections under SBR_FLAG_BF16_PROJECTION.  Goes in front of exact_f32 and of `planes`, which hold where
    // the tiled kernel cannot read the operands
    bool one_pass = false;
};
GemmMode scores_gemm_mode(const sbr_handle* h);      // sbr_step.hip, beside the engine's other modes: the projection of full_scores
// An operand as a value: element (r, c) at p[r * s_row + c * s_col]; A's rows are m and its columns k, B's rows are k and its
// columns n.  blk_Bp > 0: a tile-blocked activation [pos = t * Bp + row][col] instead (strides ignored; A: m = pos, k = col over K
// columns;  B: k = pos, n = col over N columns).
struct GemmOperand { const float* p; long s_row, s_col; int blk_Bp; };
static inline GemmOperand gemm_rowmajor(const float* p, long ld) { return GemmOperand{p, ld, 1, 0}; }        // [rows][ld] as stored
static inline GemmOperand gemm_transposed(const float* p, long ld) { return GemmOperand{p, 1, ld, 0}; }      // the transpose of a stored [cols][ld]
// What launch_gemm will do with its arguments, decided once: pure host code, no HIP call (tests/test_gemm_plan_table.py)
enum GemmKernel { GEMM_NAIVE, GEMM_X6, GEMM_F32 };
struct GemmPlan {
    GemmKernel kernel;
    int tile;                 // output tile: x6 64 or 128, or 256 for the wide 256 x 128 one (gemm_x6w_kernel); f32 64; naive 0
    int nsplit, kchunk;       // split-K slices and the K range of each (0: all of K, the naive kernel)
    int planes; float sa, sb; // x6: operand planes and scales actually used (else 0, 1, 1)
    bool reduce;              // nsplit > 1: a split-K reduction follows ...
    bool keep;                // ... or the slabs stay in ws for the consumer (may_keep and no bias)
};
GemmPlan sbr_gemm_plan(const GemmMode& mode, const GemmOperand& A, const GemmOperand& B, const float* C, long ldc, int M, int N, int K,
                       bool has_bias, const float* ws, size_t ws_floats, bool may_keep);
// ws: split-K workspace of ws_floats floats (may be NULL -> no split).
// keep_slabs != NULL: where the split-K form runs, its slabs stay in ws (slab z at ws + z * M * N, row stride N), the
// reduction is left to the consumer and *keep_slabs = their number; otherwise *keep_slabs = 0 and C holds the result
hipError_t launch_gemm(hipStream_t s, const GemmMode& mode, const GemmOperand& A, const GemmOperand& B, float* C, long ldc, int M, int N,
                       int K, const float* bias = nullptr, float* ws = nullptr, size_t ws_floats = 0, int* keep_slabs = nullptr);

// The tiled kernel (sbr_gemm_x6.hip).  sbr_gemm_x6_ok: can it run this shape on these operands with `planes` planes?  (no: a shape
// too small for its tile, no unit stride, or an operand whose rows are not 16-byte aligned, e.g. N = 3706 item columns: scalar
// loads would make the split the bottleneck).  sbr_gemm_x6_wide: does launch_gemm_x6 take the 256 x 128 tile there?  Both are
// pure host code, read by sbr_gemm_plan and by the launcher.
bool sbr_gemm_x6_ok(const GemmOperand& A, const GemmOperand& B, int M, int N, int K, bool small, int planes);
bool sbr_gemm_x6_wide(const GemmMode& mode, const GemmOperand& A, const float* C, long ldc, int M, int N, int K, int nsplit, int kchunk,
                      size_t slab_stride, bool small);
// mode: planes (0 as 3), sa, sb, no_wide.  false = not launched (sbr_gemm_x6_ok, or B2 / poll ask for what it cannot do).
// nsplit == 1: C (row stride ldc, + bias); nsplit > 1: slab z at C + z*slab_stride, row stride ldc.
bool launch_gemm_x6(hipStream_t s, const GemmMode& mode, const GemmOperand& A, const GemmOperand& B, float* C, long ldc, int M, int N,
                    int K, const float* bias, int nsplit, int kchunk, size_t slab_stride, hipError_t* err, const float* B2 = nullptr,
                    long sbk2 = 0, int n_split = 0, bool small = false, const SbrPoll* poll = nullptr);

// slabs are [z][slab_stride] with row stride ws_ld: a GEMM may fill only a column range of wider slabs
hipError_t launch_gemm_slabs(hipStream_t s, const GemmMode& mode, const GemmOperand& A, const GemmOperand& B, int M, int N, int K,
                             float* ws, int nsplit, long ws_ld, size_t slab_stride);
// same through the tiled kernel only, with the B columns >= n_split taken from B2 (row stride sbk2); false: not launched
bool launch_gemm_slabs_x6(hipStream_t s, const GemmMode& mode, const GemmOperand& A, const GemmOperand& B, int M, int N, int K,
                          float* ws, int nsplit, long ws_ld, size_t slab_stride, const float* B2, long sbk2, int n_split,
                          hipError_t* err);
// the same as a consumer of the running chain: poll.n_slabs slabs of K, poll.slab_lo[0 .. n_slabs] (device) their first rows,
// shared by n_groups persistent groups of workgroups, each of which leaves ONE partial in ws (n_groups partials to reduce)
bool launch_gemm_slabs_x6_poll(hipStream_t s, const GemmMode& mode, const GemmOperand& A, const GemmOperand& B, int M, int N, int K,
                               float* ws, int n_groups, long ws_ld, size_t slab_stride, const float* B2, long sbk2, int n_split,
                               hipError_t* err, const SbrPoll& poll);
// host side of the table: lo[0] = 0 < lo[1] < ... < lo[n] = K, n <= cap.  A slab that starts at time step t has
// max(1, floor(growth * t - 1)) k steps of 32 rows, at most max_rows / 32 (sizes scaled up until n <= cap).
int sbr_tail_slab_table(int K, int rows_per_step, int cap, double growth, int max_rows, std::vector<int>& lo);
hipError_t launch_splitk_reduce(hipStream_t s, const float* ws, int nslabs, int M, int N, float* C, long ldc,
                                const float* bias);

// dedicated dW_hid kernel: nslices slabs [Hp][GHp]; dhc != NULL: GRU compact candidate-gate array for cols >= 2*Hp
bool launch_wgrad_slabs(hipStream_t s, const float* hs, const float* dxt, const float* dhc, float* slabs, int Hp, int GHp,
                        int npos, int nslices, hipError_t* err);

// sbr_head.hip: logits + softmax / CCE + dh of a full-softmax head in one launch (C1 / C2-class catalogues); false: not served
bool sbr_head_plan(int Bp, int N, int Hp, int* CC, int* CW, size_t* lds_bytes);
// the sampled head in one launch (sbr_head.hip: head_sampled_kernel); false: shape not served, nothing launched
bool sbr_head_sampled_ok(int rows, int C, int Hp, int loss);      // (the shapes it serves: launch_head_sampled's own test, sbr_query's too)
bool launch_head_sampled(hipStream_t s, const float* h, const float* Wc, const float* bc, const float* pop, float* act, float* rowcost,
                         float* dh, int rows, int C, int Hp, int Bg, int S, int row_offset, int loss, int Bglobal, hipError_t* err,
                         unsigned long long* prof = nullptr);
bool launch_head_cce(hipStream_t s, const float* h, const float* WoutT, const float* bout, const int* tgt, const float* pop, float* dlogits,
                     float* rowcost, float* slabs, size_t slab_floats, unsigned* stats, int* fault, int Bp, int N, int Nl, int Hp, int Bglobal,
                     unsigned epoch, unsigned long long wait_ticks, int* n_slabs, hipError_t* err, unsigned long long* prof = nullptr);
// full softmax + categorical cross-entropy (rnn_one_hot.py:65-77): logits (rows,N), row stride ld, in; dlogits out in place
hipError_t launch_softmax_cce(hipStream_t s, float* logits, const float* bout, const int* target, const float* pop,
                              float* rowcost, int rows, int N, long ld, int Bglobal);
hipError_t launch_softmax_rows(hipStream_t s, float* logits, const float* bout, int rows, int N, int do_softmax);
// RNNMargin (rnn_margin.py:62-69, :112-147): logits (rows, N) raw h.W_out in, d cost / d logits out in place; target [rows][NT]
// (-1 = none), X / len: the rows' input items (weight 0 and target 0 on them when unique)
hipError_t launch_margin_loss(hipStream_t s, float* logits, const float* bout, const int* target, int NT, const int* X,
                              const int* len, int T, int F, const float* dflt, float* rowcost, int rows, int N, long ld,
                              int Bglobal, int loss, float balance, int unique);
// db[n] = sum_rows d[r][n] + reg term ; cost += reg term
hipError_t launch_colsum_bias(hipStream_t s, const float* d, int rows, int N, long ld, float* db, const float* b,
                              float reg, float* cost, float* ws /* >= 16*N floats */);
hipError_t launch_sum_cost(hipStream_t s, const float* rowcost, int rows, float* cost);
// sampled heads (sparse_lstm.py:42-54, rnn_sampling.py:68-91,137)
hipError_t launch_build_cells(hipStream_t s, const int* target, const int* samples, int Bg, int S, int* cells);
hipError_t launch_gather_rows(hipStream_t s, const float* W, const float* b, const int* cells, int C, int Hp,
                              float* Wc, float* bc);
hipError_t launch_sampled_loss(hipStream_t s, float* act, const float* bc, const float* pop, float* rowcost, int rows,
                               int Bg, int S, int row_offset, int loss, int Bglobal);
hipError_t launch_scatter_cells(hipStream_t s, float* dW, float* db, const float* dWc, const float* dbc,
                                const int* cells, int C, int Hp);
// optimizers (lasagne.updates.* [3P], update_manager.py:24-82): the dense step kernels (sbr_update.hip) take the step's rule
// (sbr_upd.h); s1 NULL where the updater has one state array
// n elements starting at p / g / s0 / s1, skipping gap_len elements after the first gap_at (two ranges, one launch)
hipError_t launch_update(hipStream_t s, const SbrUpdRule& st, float* p, float* g, float* s0, float* s1, size_t n,
                         size_t gap_at = (size_t)-1, size_t gap_len = 0);
// ... of a block whose gradient is still split-K slabs [nslabs][n] (16-byte aligned, n % 4 == 0): reduction + step in one launch
hipError_t launch_update_from_slabs(hipStream_t s, const SbrUpdRule& st, const float* ws, int nslabs, float* p, float* s0, float* s1,
                                    size_t n);
// ... of an item-indexed block of n_rows rows, reading / clearing the gradient of the rows with offs[r + 1] > offs[r] only
hipError_t launch_update_rows_aware(hipStream_t s, const SbrUpdRule& st, float* p, float* g, float* s0, float* s1, int n_rows,
                                    int row_floats, const int* offs);
// the output layer's gradient + its step in one launch; false: shape not served
bool launch_out_grad_step(hipStream_t s, const SbrUpdRule& st, const float* dlogits, const float* h_last, const float* rowcost,
                          float* cost, float* W, float* Ws0, float* Ws1, float* b, float* bs0, float* bs1, int R, int N, int Nl, int Hp,
                          hipError_t* err);
// sbr_sparse.hip: row-sparse optimizer steps (lazy catch-up) and gradient exchange for the large-catalogue blocks
struct SbrSparseRows { int npairs; size_t off[2]; int width[2]; int stride[2]; int n_rows; float *p, *g, *s0, *s1; int* last; };
// rule.a_t is not used on this path: a row kernel replays steps of several numbers and reads each one's a_t from the table
// at[t - 1], t = 1 .. n_at (sbr_adam_at; beyond it a_t == lr); early_exit: a missed Adam step's update shrinks monotonically
struct SbrSparseUpd { SbrUpdRule rule; const float* at; int n_at; int early_exit; };
hipError_t launch_sparse_catch_up_batch(hipStream_t s, const SbrSparseRows& r, const SbrSparseUpd& c, const int* X, const int* len, int T,
                                        int Bp, int F, int t_to);
hipError_t launch_sparse_catch_up_list(hipStream_t s, const SbrSparseRows& r, const SbrSparseUpd& c, const int* list, const int* n_dev,
                                       int n_host, int n_max, int t_to);
hipError_t launch_sparse_flush(hipStream_t s, const SbrSparseRows& r, const SbrSparseUpd& c, int t_to);
hipError_t launch_sparse_step_list(hipStream_t s, const SbrSparseRows& r, const SbrSparseUpd& c, const int* list, const int* n_dev,
                                   int n_host, int n_max, int t_to);
hipError_t launch_sparse_pack(hipStream_t s, const SbrSparseRows& r, const int* list, const int* n_dev, int n_host, int n_max, int* mark,
                              int epoch, int* ids_out, float* rows_out, int W, int* count);
hipError_t launch_sparse_unpack_add(hipStream_t s, const SbrSparseRows& r, const int* ids, const float* rows, int n, int W, int* cand);
hipError_t launch_sparse_unpack_add_dev(hipStream_t s, const SbrSparseRows& r, const int* ids, const float* rows, int cap, int W, int* cand);
hipError_t launch_fill(hipStream_t s, float* p, float v, size_t n);
// sbr_rank.hip: ordered top-k of any k with per-row exclusion (include/sbr_rnn.h: sbr_topk, sbr_rank)
// The one exclusion of every ranking call: the ids that `src` names for row r (sbr_device.h: ExclSources -- the caller's CSR lists,
// the row's input window, the viewed half of the row's user) leave row r of `to` (ExclCatalogue: a value at scores[r][id];
// ExclCluster: -inf at the id's place of a compact cluster row).  One workgroup of 256 per row; no source, no launch.
struct ExclSources;
template <class Sink> hipError_t launch_exclude(hipStream_t s, int rows, const ExclSources& src, const Sink& to);
// the (at most k) entries of every row that a ranking to depth k holds, in id order: keys / ids [rows][k], n_sel [rows]; returns the
// regime in *select (1: the row's keys in LDS, 2: streamed)
hipError_t launch_rank_select(hipStream_t s, const float* scores, int rows, int N, int k, unsigned* keys, int* ids, int* n_sel, int* select);
// ... sorted by key descending, id ascending, into out_ids / out_scores [rows][k] (-1 / -inf behind a row's n_sel); keys2 / ids2: the
// radix sort's second buffer pair (not read when k <= kRankSortLds); returns the regime in *sort (1: LDS bitonic, 2: radix in scratch)
hipError_t launch_rank_sort(hipStream_t s, const float* scores, int rows, int N, int k, unsigned* keys, int* ids, unsigned* keys2, int* ids2,
                            const int* n_sel, int* out_ids, float* out_scores, int* sort);
// sbr_cluster_rank.hip: ranking inside each row's item cluster (include/sbr_rnn.h: sbr_cluster_lists, sbr_cluster_rank)
// builds c's member lists if R changed since they were built (synchronises the stream once then); SBR_OK or a negative sbr_status
int sbr_cluster_build_lists(sbr_cluster* c);
// words of int scratch launch_crk_group needs behind its csel [rows]: counts [C], offsets [C + 1], row order [rows], the tile
// table [3][max_tiles] and the tile count [1]
static inline int sbr_crk_max_tiles(int rows, int C) { return rows / 16 + C; }
static inline size_t sbr_crk_group_words(int rows, int C) { return (size_t)C + (C + 1) + rows + 3 * (size_t)sbr_crk_max_tiles(rows, C) + 1; }
// counting sort of the rows by csel and the table of 16-row tiles (cluster, first place in `order`, rows)
hipError_t launch_crk_group(hipStream_t s, const int* csel, int rows, int C, int* work);
// cs[row][j] = h[row] . WoutT[members(c)[j]] + bout[...] for the tiles of `work`, -inf behind a row's list: the accumulation
// order of gemm_f32_mfma + softmax_rows_kernel, bit for bit
hipError_t launch_crk_score(hipStream_t s, const float* h, int ldh, const float* WoutT, const float* bout, int K, const int* mem_ids,
                            const int* mem_off, const int* work, int rows, int C, int lmax, float* cs);
// the second form: cs[row][j] = logits[row][members(c)[j]]
hipError_t launch_crk_gather(hipStream_t s, const float* logits, int N, const int* csel, const int* mem_ids, const int* mem_off,
                             int rows, int lmax, float* cs);
// places -> item ids, widened from kk to k columns (-1 / -inf); clu / size (nullable) [rows]: the row's cluster and its list's length
hipError_t launch_crk_translate(hipStream_t s, const int* pos, const float* psc, int kk, int k, const int* csel, const int* mem_ids,
                                const int* mem_off, int rows, int* out_ids, float* out_scores, int* size);
// sbr_cand_rank.hip: ranking inside a candidate list per row (include/sbr_rnn.h: sbr_rank_candidates, sbr_sessions_rank_candidates)
// cs[row][j] = h[row] . WoutT[cand(row)[j]] + bout[...] for the ascending lists cand_ids[cand_off[row] .. cand_off[row + 1]) of rows that
// do not share them, -inf behind a row's list: the accumulation order of gemm_f32_mfma + softmax_rows_kernel, bit for bit
hipError_t launch_cand_score(hipStream_t s, const float* h, int ldh, const float* WoutT, const float* bout, int K, const int* cand_ids,
                             const int* cand_off, int rows, int lmax, float* cs);
// launch_crk_group's words (sbr_crk_group_words(rows, 1) of them) for one cluster that all `rows` rows select, written on the host
void cand_shared_work(int rows, int* work);
// makes c->hard = f(100 R) if R changed since it was made and, with transposed, c->hardT from it; SBR_OK or a negative sbr_status
int sbr_cluster_build_hard(sbr_cluster* c, int transposed);
// sbr_eval.hip: evaluation of whole users on the device (include/sbr_rnn.h: sbr_evaluate).  A user's sequence is split in the middle
// (UserSplit above): the viewed half, the rest is the goal.
// What sbr_evaluate reads of a dataset (sbr_batch.hip owns the struct): the sequences as uploaded -- never the noised copy --, the
// host copy of the offsets for the argument checks, and `goal`: per user the goal items[off + half .. off + L) sorted ascending, at
// the same places of a second array (its viewed places are not written).  Built on the first call, freed with the dataset.
struct SbrEvalView {
    int64_t n_users; int n_items; hipStream_t stream;
    const int *items, *rate, *goal; const long long* off; const int64_t* h_off;
};
int sbr_dataset_eval_view(sbr_dataset* d, SbrEvalView* v, int with_goal);      // with_goal = 0: no `goal`, nothing allocated or copied
// rows [0, rows) of the batch buffers from users[0 .. rows): the last min(T, half) viewed items left-aligned (+ n_items + rating index
// with F == 2, as bb_pack_kernel writes it), the length, popularity 1; rows [rows, Bp): index 0, length 0, popularity 1
hipError_t launch_ev_pack(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int Bp, int T, int F, int* X, int* lengths, float* pop);
// per row r of ids [rows][k] (ordered top-k, -1 behind the filled places): n_pred, hits, first_hit [rows], mask [rows][(k + 31) / 32]
// (NULL: not written), item_hits [N] += 1 per hit (NULL: not counted)
hipError_t launch_ev_hits(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int k, const int* ids, int* n_pred, int* hits,
                          int* first_hit, unsigned* mask, int* item_hits);
// rank[r][j] of goal item j of users[r] in the complete ranking of scores[r] (include/sbr_rnn.h: sbr_evaluate_ranks) at
// ranks[goal_off[r] + j], -1 for an item that is never ranked; n_rankable [rows]; returns the regime in *form (1: the row's keys in LDS,
// 2: streamed)
hipError_t launch_ev_goal_rank(hipStream_t s, const SbrEvalView& v, const int* users, const long long* goal_off, int rows, int N,
                               const float* scores, int* ranks, int* n_rankable, int* form);
// sbr_evaluate_positions (include/sbr_rnn.h; UserPrefix above).  The rows fed: the first min(L - 1, T) items of every user, otherwise
// what launch_ev_pack writes
hipError_t launch_ev_pack_prefix(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int Bp, int T, int F, int* X, int* lengths, float* pop);
// first[r][q] = 1 iff the item at place q of row r of X does not occur at a place in front of q (q < lengths[r]; the rest is not written)
hipError_t launch_ev_first_seen(hipStream_t s, const int* X, const int* lengths, int rows, int T, int F, int* first);
// positions p = p0 .. p0 + slots - 1 of every row r with p <= lengths[r]: the rank of x_p = items[off[users[r]] + p] among the scores
// scores[(p - p0) * slot_stride + r * N ..] and the row's rankable items, at pos_off[r] + p - min_history of ranks / n_rankable;
// exclude_prefix: the items flagged in first[r][0 .. p) are taken out
hipError_t launch_ev_next_rank(hipStream_t s, const SbrEvalView& v, const int* users, const long long* pos_off, const int* X, const int* lengths,
                               const int* first, int rows, int T, int F, int N, int p0, int slots, int min_history, int exclude_prefix,
                               const float* scores, size_t slot_stride, int* ranks, int* n_rankable, int* form);
// sbr_evaluate_logprob / sbr_evaluate_positions_logprob (include/sbr_rnn.h): the log-probability of launch_ev_goal_rank's
// and launch_ev_next_rank's goal items under the softmax over the rankable items of the same score rows, at the same places of logp;
// log_z (NULL: not written) [rows], or at the places of logp for the positions.  The positions form WRITES -inf at the ids of the
// prefix into its score rows when exclude_prefix is set.  *form: 1 16-byte loads, 2 4-byte loads; the bits do not depend on it.
hipError_t launch_ev_goal_logprob(hipStream_t s, const SbrEvalView& v, const int* users, const long long* goal_off, int rows, int N,
                                  const float* scores, float* logp, float* log_z, int* form);
hipError_t launch_ev_next_logprob(hipStream_t s, const SbrEvalView& v, const int* users, const long long* pos_off, const int* X, const int* lengths,
                                  int rows, int T, int F, int N, int p0, int slots, int min_history, int exclude_prefix, float* scores,
                                  size_t slot_stride, float* logp, float* log_z, int* form);
// ... and the same reduction on any rows [rows][ld] of device scores, goal_ids [rows][goals_per_row] (sbr_debug_row_logprob)
hipError_t launch_debug_row_logprob(hipStream_t s, const float* scores, size_t ld, int rows, int N, const int* goal_ids, int goals_per_row,
                                    float* logp, float* log_z, int* form);
// sbr_eval_cand.hip: goal items ranked among a candidate set per user (include/sbr_rnn.h: sbr_evaluate_candidates)
// What ev_cand_build_kernel reads and writes for the rows of one chunk.  The candidates of row r are either the explicit list
// cand_ids[cand_off[r] .. cand_off[r + 1]) (strictly ascending) or, with cand_ids == nullptr, n_neg negatives drawn by the rule above.
// cap_off [rows + 1]: where row r's merged list may lie, cap_off[r + 1] - cap_off[r] >= its candidates + its goal items (the host's bound).
struct EvCandBuild {
    const int* users; int rows, N;
    const int* cand_ids; const int* cand_off;
    int n_neg; unsigned long long seed; const double* cdf; int hash_slots;
    int* negatives;                    // nullptr, or [rows][n_neg]: the accepted items in draw order, -1 behind the last
    const long long* cap_off;
    // written: the device CSR launch_cand_score / launch_crk_gather read -- moff [rows + 1] = cap_off rebased to 0, mem: per row its
    // candidates and distinct goal items in the catalogue merged strictly ascending, mlen[r] of them, the rest of the row's capacity
    // padded with a copy of its last id (0 for an empty row); flag per entry: 1 candidate, 0 goal item only, 2 padding; csel[r] = r
    int* moff; int* mem; unsigned char* flag; int* mlen; int* csel;
};
hipError_t launch_ev_cand_build(hipStream_t s, const SbrEvalView& v, const EvCandBuild& a);
// ranks[goal_off[r] + p]: the rankable candidates (flag 1) of row r that stand before goal item p in sbr_rank's order among the compact
// scores cs [rows][lmax] (place j of row r: item mem[moff[r] + j]), -1 for a goal item that is never ranked; n_cand [rows]: the rankable
// candidates.  The items exclude_mode names (SBR_EVAL_EXCL_VIEWED / _WINDOW, read from the dataset's CSR) are set to -inf in cs first.
hipError_t launch_ev_cand_place(hipStream_t s, const SbrEvalView& v, const int* users, const long long* goal_off, int rows, int T, int N,
                                int exclude_mode, const int* mem, const int* moff, const unsigned char* flag, const int* mlen, float* cs,
                                int lmax, int* ranks, int* n_cand);
// sbr_cluster_eval.hip: what sbr_cluster_evaluate needs beyond the kernels above (include/sbr_rnn.h)
hipError_t launch_cev_transpose(hipStream_t s, const float* hard, int N, int C, float* hardT);
// prod[r][i] = softmax(logits[r])[i] * hardT[csel[r]][i] (logits: biased, untouched by any exclusion), then with zero_fed +0.0 at the
// items fed of users[r]
hipError_t launch_cev_product(hipStream_t s, const SbrEvalView& v, const int* users, int rows, int T, int N, int C, int zero_fed,
                              const float* logits, const int* csel, const float* hardT, float* prod);
// use[c] += rows of csel[0 .. n) that selected c (integer atomics)
hipError_t launch_cev_use(hipStream_t s, const int* csel, long long n, int C, int* use);
