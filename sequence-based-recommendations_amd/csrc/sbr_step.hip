// The training step of libsbr_rnn.so (include/sbr_rnn.h): sbr_forward, sbr_loss_backward_output, sbr_backward_recurrent,
// sbr_apply_update, the single-call forms sbr_train_step / sbr_train_step_lagged and sbr_cost_lagged.  Host code only: which kernel goes on which
// stream in which order; the arithmetic lives in the kernels.  Every launch recipe that more than one road of the step takes is
// written once, in the first half of this file (kernel arguments, sort arrays, timing marks, optimizer steps, row-sparse blocks,
// the GEMMs around a recurrent layer); the phases below are built from them.  What the rest of the engine (sbr_api.hip) needs of
// the step is declared in sbr_common.h.
#include "sbr_common.h"
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>

// ---------------------------------------------------------------------------------------
// kernel arguments, plans, epochs
// ---------------------------------------------------------------------------------------
// slot k of the profile buffer: 0 the forward chain, 1 the backward chain, 2 the one-launch head (tools/rec_prof.py, cl_prof.py, head_prof.py)
static inline unsigned long long* prof_slot(const sbr_handle* h, int k) {
    return (unsigned long long*)h->A(h->lay.a_prof) + (size_t)k * (h->lay.Bp / 16) * 16 * 8;
}
// layer l without a batch: its sizes, the engine's switches and flags, where its activations lie -- what sbr_rec_plan reads
static RecArgs rec_shape(const sbr_handle* h, int l) {
    const Layout& y = h->lay; const LayerLayout& ly = y.layer[l];
    RecArgs a; memset(&a, 0, sizeof(a));
    a.cell = y.cfg.cell; a.T = y.T; a.Bp = y.Bp; a.H = ly.H; a.Hp = ly.Hp; a.G = y.G;
    a.n_in = ly.n_in_p;
    a.clip = y.cfg.grad_clip;
    a.rpt = h->rpt; a.x6_pipe = h->sw.x6_pipe; a.x6_f16 = h->sw.x6_f16; a.x6_f16_bwd = h->sw.x6_f16_bwd;
    a.cl16 = h->sw.cl16; a.c16_two_level = h->sw.c16_two_level;
    a.hs = h->A(ly.a_hs); a.cs = h->A(ly.a_cs);
    for (int k = 0; k < 4; ++k) a.g[k] = h->A(ly.a_g[k]);
    if (ly.Hp == 256 || ly.Hp == 512) { a.xh = h->A(ly.a_xh); a.pring = h->A(ly.a_pring); }
    a.f32_mfma = (y.cfg.flags & SBR_FLAG_F32_MFMA) ? 1 : 0;
    a.prof = (y.cfg.flags & SBR_FLAG_PROFILE_REC) ? prof_slot(h, 0) : nullptr;
    a.cluster = h->sw.cluster; a.cl_linear = h->sw.cl_linear;
    a.relu = (y.cfg.cell == SBR_CELL_VANILLA && (l / y.D > 0 || y.E)) ? 1 : 0;   // stock RecurrentLayer: rectify [3P]
    return a;
}
// layer l's kernel arguments for the current batch; advances the cluster kernels' exchange epoch (unique per launch)
static RecArgs rec_args(sbr_handle* h, int l) {
    const Layout& y = h->lay; const LayerLayout& ly = y.layer[l];
    RecArgs a = rec_shape(h, l);
    a.len = h->blen;
    a.xt = h->A(ly.a_xt); a.Whid = h->P(ly.p_Whid); a.peep = h->P(ly.p_peep);
    a.cinit = h->P(ly.p_cinit); a.hinit = h->P(ly.p_hinit);
    a.dxt = h->A(ly.a_dxt); a.dhi = h->A(ly.a_dhi); a.part = h->A(ly.a_part);
    a.xt_blocked = 0;
    a.t_lo = 0; a.t_hi = y.T; a.chunk = 0; a.state = h->A(ly.a_state);
    a.fault = (int*)h->A(y.a_fault);
    a.clx = (int*)h->A(y.a_clx); a.epoch = (++h->cl_epoch) & 0x07FFFFFF;
    return a;
}
static bool simple_rec(const sbr_handle* h) { return h->lay.cfg.flags & SBR_FLAG_SIMPLE_REC; }
// The plans of all layers, made once inside sbr_create.  dh_ext as the BPTT launch will have it (bptt_args); the step lets the
// forward kernel gather W_in's rows where the input is one index per step without an embedding in front (layer0_input).
void plan_layers(sbr_handle* h) {
    const Layout& y = h->lay;
    for (int l = 0; l < y.L * y.D; ++l) {
        RecArgs a = rec_shape(h, l);
        if (l / y.D < y.L - 1) a.dh_ext = h->A(y.layer[l].a_dhext);
        h->plan[l] = sbr_rec_plan(a, simple_rec(h), l / y.D == 0 && !y.E && y.F == 1 && h->sw.fuse_gather);
    }
}
static const RecPlan& plan_of(const sbr_handle* h, const LayerLayout& ly) { return h->plan[&ly - h->lay.layer]; }
// Operand planes of the dense GEMMs around the recurrent layers (layer >= 2 input projection and its backward pair, the logits):
// their operands are hidden states in [-1, 1] (not behind a rectifier), weights, and -- in the backward pair -- gate gradients
// that have passed the reference's clip at +-100 (recurrent_layers.py:19): the two-plane fp16 split, three MFMAs per product, f32-class
// (SBR_GEMM_F16=0: bf16x6 as in rounds 1-3).  SBR_FLAG_BF16_LAYERS: plain bf16 operands, one MFMA (BASELINE configs[4]).
// Every GemmMode of an engine is built here, from its flags and switches; the launchers keep nothing between calls.
bool simple_gemm(const sbr_handle* h) { return h->lay.cfg.flags & SBR_FLAG_SIMPLE_GEMM; }
// nothing stated: operands of unknown range (behind an embedding, loss gradients, the sampled heads) -- bf16x6, or what the flags say
static GemmMode gemm_mode(const sbr_handle* h, int planes = 0, float sa = 1.0f, float sb = 1.0f) {
    return GemmMode{simple_gemm(h), (h->lay.cfg.flags & SBR_FLAG_F32_MFMA) != 0, planes, sa, sb};
}
// the fp16 split where it is allowed; grad_a / grad_b: that side carries gradients (scaled by 512 on the way in)
static GemmMode layer_gemm_f16(const sbr_handle* h, bool grad_a, bool grad_b) {
    const Layout& y = h->lay;
    if (!h->sw.gemm_f16 || y.cfg.cell == SBR_CELL_VANILLA) return gemm_mode(h);
    if ((grad_a || grad_b) && !(y.cfg.grad_clip > 0.0f && y.cfg.grad_clip <= 100.0f)) return gemm_mode(h);
    return gemm_mode(h, 2, grad_a ? 512.0f : 1.0f, grad_b ? 512.0f : 1.0f);
}
static GemmMode layer_gemm_mode(const sbr_handle* h, bool grad_a, bool grad_b) {      // layer >= 2: input projection and its backward pair
    return (h->lay.cfg.flags & SBR_FLAG_BF16_LAYERS) ? gemm_mode(h, 1) : layer_gemm_f16(h, grad_a, grad_b);
}
// The projections onto the catalogue take one pass of plain bf16 under SBR_FLAG_BF16_PROJECTION.  The step's logits (h in [-1, 1] x
// weights), and full_scores': always the exact-f32 kernel otherwise -- a row's scores (hence its ranked ids) must not depend on how many
// rows share the call (the bf16x6 kernel takes over at >= 96 rows and rounds differently; the one-pass kernel serves any number alike)
static GemmMode projection_mode(const sbr_handle* h, bool scoring) {
    const bool bf16p = (h->lay.cfg.flags & SBR_FLAG_BF16_PROJECTION) && !simple_gemm(h);
    GemmMode m = (bf16p || scoring) ? gemm_mode(h) : layer_gemm_f16(h, false, false);
    m.one_pass = bf16p; m.exact_f32 |= scoring;
    return m;
}
GemmMode scores_gemm_mode(const sbr_handle* h) { return projection_mode(h, true); }
// the weight-gradient slabs: hs^T . gradients, scaled where the split is taken (WgradPlan.f16)
static GemmMode wgrad_gemm_mode(const sbr_handle* h, bool f16) { return gemm_mode(h, f16 ? 2 : 3, 1.0f, f16 ? 512.0f : 1.0f); }
// Does a step over `rows` batch rows take the one-launch sampled head (head_sampled_kernel)?  Asked by the step and by sbr_query.
bool head_sampled_taken(const sbr_handle* h, int rows) {
    const Layout& y = h->lay;
    return h->sw.head_fuse && !simple_gemm(h) && y.D == 1 && !(y.cfg.flags & SBR_FLAG_F32_MFMA) &&
           sbr_head_sampled_ok(rows, y.C, y.HLt, y.cfg.loss);
}
// Overlapped step tail, planned once inside sbr_create (behind plan_layers): time chunks of a training step (h->tail_chunks, 0 = not
// taken), steps per chunk and the chunks' bounds.  Taken for a single index-input layer served by rec_bwd_x6p's progress-publishing
// form, dense updates, the bf16x6 weight-gradient GEMM and one BPTT launch.
void plan_tail(sbr_handle* h) {
    const Layout& y = h->lay;
    h->tail_chunks = h->tail_ch = 0;
    if (!h->sw.tail_overlap || y.tail_keys < 2 || y.n_sparse || h->sw.bwd_chunks != 1) return;
    if (!h->plan[0].tail_ok || simple_gemm(h) || (y.cfg.flags & SBR_FLAG_ATOMIC_SCATTER)) return;      // (tail_ok: never triage or exact-f32 kernels)
    int nc = std::min(std::min(y.tail_keys, kTailChunksMax), y.T / 16);
    if (nc < 2) return;
    const int ch = (y.T + nc - 1) / nc;
    nc = (y.T + ch - 1) / ch;
    if (nc < 2) return;
    h->tail_chunks = nc; h->tail_ch = ch;
    // Chunk bounds.  The scatter-add of a time chunk can start when the chain has left it, and the chain leaves chunk 0 last:
    // with equal chunks an eighth of the step's entries waits for the chain's end (30 - 45 us of polling waves behind it,
    // profiles/round3_c_timeline.txt).  So the chunks near t = 0 are small -- 1, 3, 7, 18 ... steps (powers of sbr_tail_geom,
    // 2.6; <= 1: equal chunks) -- until a power exceeds the equal share of what is left, which the remaining chunks then
    // take: at T = 200 and eight chunks 1, 3, 7, 18, 42, 43, 43, 43 steps (the consumers still start after a fifth of the chain).
    // At most half of the chunks are small ones.
    const double geom = sbr_tail_geom(h->sw.tail_scatter_lds);
    SbrTChunks& tc = h->tail_bounds;
    tc.n = nc;
    tc.lo[0] = 0;
    // LDS-row scatter-add (launch_scatter_lds_poll): a unit walks the chunks one after the other, so what counts is that chunk c is
    // done when chunk c - 1 is released and that ONE round of rows is left behind the chain: the last chunk has kTailFirst
    // steps (6: ~8 entries per unit) and the sizes grow by sbr_tail_geom (1.6 here): 6, 10, 15, 25, then equal shares.
    double pw = h->sw.tail_scatter_lds ? (double)kTailFirst : 1.0;
    for (int c = 0; c < nc; ++c) {
        const int rem = y.T - tc.lo[c], left = nc - c;
        const int share = (rem + left - 1) / left;
        const int n_small = nc >= 4 ? nc / 2 : (nc - 1) / 2;
        int sz = (geom > 1.0 && c < n_small) ? std::min(share, std::max(1, (int)(pw + 0.5))) : (geom > 1.0 ? share : std::min(rem, ch));
        if (c == nc - 1) sz = rem;
        sz = std::max(1, std::min(sz, rem - (left - 1)));            // every later chunk keeps at least one step
        tc.lo[c + 1] = tc.lo[c] + sz;
        pw *= geom > 1.0 ? geom : 1.0;
    }
    for (int c = nc; c <= SBR_TCHUNKS_MAX; ++c) tc.lo[c] = y.T;
}

// The one place where the epoch of the chain's progress words advances: once per step, in front of whatever is launched first
// with it -- the gate at the head of the side stream (sbr_loss_backward_output) or the chain (sbr_backward_recurrent).
static int tail_next_epoch(sbr_handle* h) {
    h->prog_epoch = (h->prog_epoch + 1) & 0x7FFFF; if (!h->prog_epoch) h->prog_epoch = 1;
    return h->prog_epoch;
}
// Step boundary (kStepJoinGate / kStepForkGate): the epoch of the completion words / of the start word advances once per step that
// publishes them, by the same rule -- a word the step before left carries the epoch before, never this one, and never 0 (the
// words start as zeros).  Both timing marks of the boundary (0: in front of the forward, 6: between the two joins) are event
// records on the main stream at the very points the gates take the events from: with either of them on, the events stay.
static int step_next_epoch(int* e) { *e = (*e + 1) & 0x7FFFFFFF; if (!*e) *e = 1; return *e; }
static bool step_boundary_marks(const sbr_handle* h) { return h->timing && (h->timing_marks & ((1u << 0) | (1u << 6))); }
// the chain's progress words of this step's overlapped tail, one per wave of rec_bwd_x6p
static int* tail_words(sbr_handle* h, int* nwaves) {
    *nwaves = (h->lay.Bp / h->rpt) * 8;
    return (int*)h->A(h->lay.a_prog);
}

// ---------------------------------------------------------------------------------------
// the counting sort of the batch's ids
// ---------------------------------------------------------------------------------------
// one direction's sort arrays: 0 the batch's ids, 1 (--r_bi without --r_emb) the reversed ids of the backwards layer
SbrSortKeys sort_keys(const sbr_handle* h, int dir) {
    const Layout& y = h->lay;
    if (dir) return {(int*)h->A(y.a_s2cnt), (int*)h->A(y.a_s2off), (int*)h->A(y.a_s2cur), (int*)h->A(y.a_s2sid), (int*)h->A(y.a_s2pos)};
    return {(int*)h->A(y.a_scnt), (int*)h->A(y.a_soff), (int*)h->A(y.a_scur), (int*)h->A(y.a_sid), (int*)h->A(y.a_spos)};
}
// entries of the sort: every (position, feature) pair of the padded batch
static inline int sort_entries(const Layout& y) { return y.T * y.Bp * y.F; }

// the time-chunked sort of an overlapped tail and (LDS-row scatter-add) the ids' running cost, on the second side stream, which consumes them
static int tail_sort(sbr_handle* h) {
    const Layout& y = h->lay; const SbrSortKeys k = sort_keys(h, 0);
    SBR_LAUNCH(launch_scatter_sort(h->side2, h->bX, h->blen, y.T, y.Bp, y.F, y.cfg.input_size, k.cnt, k.off, k.cur, k.sid, k.pos, 0,
                                   h->tail_ch, h->st.tail_nc, &h->tail_bounds, &h->scnt_zero_n));
    if (h->scat.tail == SCAT_LDS)
        SBR_LAUNCH(launch_scatter_cost_scan(h->side2, k.off, (int*)h->A(y.a_sP), y.cfg.input_size, h->st.tail_nc, h->scat));
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// timing marks
// ---------------------------------------------------------------------------------------
// sbr_chain_times: events around one chain launch (dir 0 = forward, 1 = backward); `which` 0 in front of it, 1 behind it
static inline void chain_mark(sbr_handle* h, hipStream_t st, int dir, int which) {
    if (!h->chain_timing || h->ch_n >= sbr_handle::kChain) return;
    hipEvent_t& e = h->ev_ch[h->ch_n][which];
    if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return; }
    (void)hipEventRecord(e, st);
    if (which == 1) { h->ch_dir[h->ch_n] = (unsigned char)dir; h->ch_n += 1; }
}
#define SBR_LAUNCH_CHAIN(DIR, STREAM, CALL) do { chain_mark(h, STREAM, DIR, 0); SBR_LAUNCH(CALL); chain_mark(h, STREAM, DIR, 1); } while (0)

// is timing mark i of the step in flight recorded?
static inline bool mark_live(const sbr_handle* h, int i) { return h->timing && ((h->timing_marks >> i) & 1) && h->ev[h->ring_cur][i]; }
static inline void mark_on(sbr_handle* h, int i, hipStream_t st) {
    if ((h->st.marks_shared >> i) & 1) return;              // this step's mark i was recorded by record_shared
    if (mark_live(h, i)) (void)hipEventRecord(h->ev[h->ring_cur][i], st);
}
void mark(sbr_handle* h, int i) { mark_on(h, i, h->stream); }
// An event record costs the stream ~6 us before its next kernel starts (measured: profiles/round1_i_timeline.txt), so
// where a cross-stream event and a timing mark fall on the same point of the main stream ONE record serves both: the
// side stream waits on the timing event.  Returns the event to wait on.
static inline hipEvent_t record_shared(sbr_handle* h, hipEvent_t plain, int mk) {
    if (mk >= 0 && mark_live(h, mk)) {
        (void)hipEventRecord(h->ev[h->ring_cur][mk], h->stream);
        h->st.marks_shared |= 1u << mk;
        return h->ev[h->ring_cur][mk];
    }
    (void)hipEventRecord(plain, h->stream);
    return plain;
}

// ---------------------------------------------------------------------------------------
// optimizer steps.  The step in flight is number step_count + 1 until sbr_apply_update has completed (Adam's t).
// ---------------------------------------------------------------------------------------
static inline long step_no(const sbr_handle* h) { return (long)h->step_count + 1; }
static inline float* state1(const sbr_handle* h, size_t off) { return h->lay.n_state_arrays > 1 ? h->St(1, off) : nullptr; }
static inline SbrUpdRule upd_rule(const sbr_handle* h) { return sbr_upd_rule(h->lay.cfg, step_no(h)); }
// floats [lo, hi) of the parameter section, without the gap_len floats that follow the first gap_at of them (two ranges, one launch)
static hipError_t step_range(sbr_handle* h, hipStream_t st, size_t lo, size_t hi, size_t gap_at = (size_t)-1, size_t gap_len = 0) {
    if (hi <= lo) return hipSuccess;
    return launch_update(st, upd_rule(h), h->P(lo), h->Gd(lo), h->St(0, lo), state1(h, lo), hi - lo - gap_len, gap_at, gap_len);
}
// ... n floats at lo whose gradient is still n_slabs split-K slabs in ws: reduction + step in one launch
static hipError_t step_from_slabs(sbr_handle* h, hipStream_t st, const float* ws, int n_slabs, size_t lo, size_t n) {
    return launch_update_from_slabs(st, upd_rule(h), ws, n_slabs, h->P(lo), h->St(0, lo), state1(h, lo), n);
}
// ... layer 0's index-input block, reading / clearing the gradient of the rows this batch touched only (the plain-key sort's offsets)
static hipError_t step_rows_aware(sbr_handle* h, hipStream_t st) {
    const Layout& y = h->lay; const size_t lo = y.layer[0].p_Win;
    return launch_update_rows_aware(st, upd_rule(h), h->P(lo), h->Gd(lo), h->St(0, lo), state1(h, lo), y.cfg.input_size,
                                    y.G * y.layer[0].Hp, sort_keys(h, 0).off);
}
// ... the dense head: its gradient from dlogits, its step and the batch cost in one launch; false: shape not served
static bool step_out_grad(sbr_handle* h, hipStream_t st, const float* lg, const float* hl, int R, int Nl, hipError_t* err) {
    const Layout& y = h->lay;
    return launch_out_grad_step(st, upd_rule(h), lg, hl, h->A(y.a_rowcost), h->cost_ptr(), h->P(y.p_WoutT), h->St(0, y.p_WoutT),
                                state1(h, y.p_WoutT), h->P(y.p_bout), h->St(0, y.p_bout), state1(h, y.p_bout), R, y.N, Nl, y.HLt, err);
}

// ---------------------------------------------------------------------------------------
// row-sparse blocks (sbr_sparse.hip)
// ---------------------------------------------------------------------------------------
SbrSparseRows sparse_rows(sbr_handle* h, int b) {
    const SparseBlockLayout& sb = h->lay.sparse[b];
    SbrSparseRows r; memset(&r, 0, sizeof(r));
    r.npairs = sb.npairs; r.n_rows = sb.n_rows;
    for (int k = 0; k < sb.npairs; ++k) { r.off[k] = sb.off[k]; r.width[k] = sb.width[k]; r.stride[k] = sb.stride[k]; }
    r.p = h->P(0); r.g = h->Gd(0); r.s0 = h->St(0, 0); r.s1 = h->lay.n_state_arrays > 1 ? h->St(1, 0) : nullptr;
    r.last = (int*)h->A(sb.a_last);
    return r;
}
SbrSparseUpd sparse_upd(sbr_handle* h) {
    SbrSparseUpd u; u.rule = upd_rule(h);
    u.at = h->lay.n_at ? h->A(h->lay.a_at) : nullptr; u.n_at = h->lay.n_at; u.early_exit = h->lay.adam_early_exit;
    return u;
}
// the sampled head's block (W_out^T rows + b_out), or -1
static int sparse_out_block(const Layout& y) {
    int kb = -1;
    for (int b = 0; b < y.n_sparse; ++b) if (y.sparse[b].kind == 1) kb = b;
    return kb;
}
SbrSparseIds sparse_ids(const sbr_handle* h, int b) {
    const Layout& y = h->lay; const SbrSortKeys k = sort_keys(h, 0);
    if (y.sparse[b].kind == 0) return {k.sid, k.off + y.cfg.input_size, 0, sort_entries(y)};
    return {(const int*)h->A(y.a_cells), nullptr, y.C, y.C};
}
// this step's row step of block b over the ids in `c`: its own (sparse_ids), or the candidates gathered from every rank
static hipError_t step_rows(sbr_handle* h, hipStream_t st, int b, const SbrSparseIds& c) {
    return launch_sparse_step_list(st, sparse_rows(h, b), sparse_upd(h), c.list, c.n_dev, c.n_host, c.n_max, (int)step_no(h));
}
// block b's rows among `c` current through the last applied step, before the step reads them
static hipError_t catch_up_rows(sbr_handle* h, hipStream_t st, int b, const SbrSparseIds& c) {
    return launch_sparse_catch_up_list(st, sparse_rows(h, b), sparse_upd(h), c.list, c.n_dev, c.n_host, c.n_max, (int)h->step_count);
}

// ---------------------------------------------------------------------------------------
// the GEMMs and reductions around one recurrent layer, shared by the one-direction road and --r_bi
// ---------------------------------------------------------------------------------------
// xt = inp . W_in + b for a dense input [T * Bp][n_in_p]: the flattened embeddings, or the outputs of the level below
// (Lasagne precompute_input [3P], recurrent_layers.py:94-104)
static hipError_t input_projection(sbr_handle* h, const LayerLayout& ly, const float* inp, const GemmMode& mode) {
    const Layout& y = h->lay; const int GHp = y.G * ly.Hp;
    return launch_gemm(h->stream, mode, gemm_rowmajor(inp, ly.n_in_p), gemm_rowmajor(h->P(ly.p_Win), GHp), h->A(ly.a_xt), GHp,
                       y.T * y.Bp, GHp, ly.n_in_p, h->P(ly.p_b));
}
// Layer 0's input of the forward pass.  Index input: the rows of W_in gathered inside the forward kernel (ra is told where from),
// or by a launch of their own.  --r_emb: `emb`, the flattened embeddings of this direction, through a dense input projection.
static int layer0_input(sbr_handle* h, RecArgs& ra, const LayerLayout& ly, const int* idx, const float* emb) {
    const Layout& y = h->lay;
    if (y.E) { SBR_LAUNCH(input_projection(h, ly, emb, gemm_mode(h))); return SBR_OK; }
    if (plan_of(h, ly).fuse_gather) {
        ra.gX = idx; ra.gWin = h->P(ly.p_Win); ra.gbias = h->P(ly.p_b);   // gathered inside the forward kernel
    } else {
        SBR_LAUNCH(launch_gather_xt(h->stream, h->P(ly.p_Win), h->P(ly.p_b), idx, h->A(ly.a_xt), y.T, y.Bp, y.F, y.G * ly.Hp, h->n_rows));
    }
    return SBR_OK;
}
// the bias / peephole / initial-state gradients from the n partial blocks a layer's BPTT launches left
static hipError_t reduce_partials(sbr_handle* h, hipStream_t st, const LayerLayout& ly, const RecArgs& a, int n) {
    const Layout& y = h->lay;
    return launch_rec_reduce_partials(st, a.part, n, y.G, ly.Hp, y.cfg.cell, h->Gd(ly.p_b), h->Gd(ly.p_peep), h->Gd(ly.p_cinit),
                                      h->Gd(ly.p_hinit));
}
// the plain dW_hid = hs^T . d hid_input on the main stream (hs slot t = the state before step t); GRU: hid_input grad = [dxt_r | dxt_u | dhi_c]
static int whid_grad_gemm(sbr_handle* h, const LayerLayout& ly, const RecArgs& a) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    const int GHp = y.G * ly.Hp, TB = y.T * y.Bp;
    const GemmMode mode = gemm_mode(h);
    const GemmOperand hsT = gemm_transposed(h->A(ly.a_hs), ly.Hp);
    float* dWhid = h->Gd(ly.p_Whid); float* ws = h->A(y.a_ws);
    if (y.cfg.cell == SBR_CELL_GRU) {
        SBR_LAUNCH(launch_gemm(s, mode, hsT, gemm_rowmajor(a.dxt, GHp), dWhid, GHp, ly.Hp, 2 * ly.Hp, TB, nullptr, ws, y.ws_floats));
        SBR_LAUNCH(launch_gemm(s, mode, hsT, gemm_rowmajor(a.dhi, ly.Hp), dWhid + 2 * ly.Hp, GHp, ly.Hp, ly.Hp, TB, nullptr, ws, y.ws_floats));
    } else {
        SBR_LAUNCH(launch_gemm(s, mode, hsT, gemm_rowmajor(a.dxt, GHp), dWhid, GHp, ly.Hp, GHp, TB, nullptr, ws, y.ws_floats));
    }
    return SBR_OK;
}
// dense input [T * Bp][n_in_p]: dW_in = inp^T . dxt, d_inp = dxt . W_in^T.  hinted: between recurrent layers both operands' ranges
// are known (layer_gemm_mode); behind the embedding they are not
static int input_grads_dense(sbr_handle* h, const LayerLayout& ly, const RecArgs& a, const float* inp, float* d_inp, bool hinted) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    const int GHp = y.G * ly.Hp, TB = y.T * y.Bp;
    const GemmOperand dxt = gemm_rowmajor(a.dxt, GHp);
    SBR_LAUNCH(launch_gemm(s, hinted ? layer_gemm_mode(h, false, true) : gemm_mode(h), gemm_transposed(inp, ly.n_in_p), dxt, h->Gd(ly.p_Win),
                           GHp, ly.n_in_p, GHp, TB, nullptr, h->A(y.a_ws), y.ws_floats));
    SBR_LAUNCH(launch_gemm(s, hinted ? layer_gemm_mode(h, true, false) : gemm_mode(h), dxt, gemm_transposed(h->P(ly.p_Win), GHp), d_inp,
                           ly.n_in_p, TB, ly.n_in_p, GHp));
    return SBR_OK;
}
// the scatter-add of the F*T*B embedding-gradient rows in a_demb into dW_emb (EmbeddingLayer gradient: duplicates accumulate [3P])
static int emb_grad_scatter(sbr_handle* h) {
    const Layout& y = h->lay; const SbrSortKeys k = sort_keys(h, 0);
    SBR_HIP(hipStreamWaitEvent(h->stream, h->ev_sort, 0));
    SBR_LAUNCH(launch_scatter_reduce(h->stream, h->Gd(y.p_Emb), h->A(y.a_demb), k.sid, k.pos, k.off, y.cfg.input_size, sort_entries(y),
                                     y.Ep, y.Bp, h->scat.reduce));
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// joining the side streams
// ---------------------------------------------------------------------------------------
// The side stream carries everything that only feeds the optimizer (output-layer weight/bias gradients, the cost
// scalar, the counting sort for the embedding scatter, the weight-gradient GEMM of finished BPTT chunks) so that
// the main stream holds nothing but the dependent chain  logits -> softmax -> dh -> BPTT chunks -> scatter.
int side_join(sbr_handle* h) {
    if (h->tail_join_pending) {      // overlapped tail of a phase-by-phase step: both consumer streams
        SBR_HIP(hipStreamWaitEvent(h->stream, h->ev_tail2, 0));
        SBR_HIP(hipStreamWaitEvent(h->stream, h->ev_tail, 0));
        h->tail_join_pending = false; h->side_pending = false;
    }
    if (h->side_pending) {
        SBR_HIP(hipEventRecord(h->ev_join, h->side));
        SBR_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        h->side_pending = false;
    }
    return SBR_OK;
}
extern "C" int sbr_set_deferred_join(sbr_handle* h, int on) {
    CHECK_ARG(h, "null handle");
    h->deferred_join = on != 0;
    return SBR_OK;
}
extern "C" int sbr_join_side(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    return side_join(h);
}

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
// Sampled heads with lazily stepped W_out rows: which cells the step samples depends on the batch only, and catching their
// rows up is a chain of dependent replays per row (C3: 81 us, C5: 94 us for 288 rows) that sat on the main stream between the
// forward chain and the head.  It runs now on the side stream, beside the forward chain; sbr_loss_backward_output waits for
// its event (long complete by then).  SBR_SPARSE_OUT_EARLY=0: as before.  *forked: ev_fork was recorded on the main stream.
static int early_cells(sbr_handle* h, bool* forked) {
    const Layout& y = h->lay;
    *forked = false;
    if (!(h->sw.sparse_out_early && sparse_lazy(h) && y.S > 0 && y.cfg.loss != SBR_LOSS_CCE && !SBR_LOSS_IS_MARGIN(y.cfg.loss))) return SBR_OK;
    const int kb = sparse_out_block(y);
    if (kb < 0) return SBR_OK;
    SBR_HIP(hipEventRecord(h->ev_fork, h->stream)); *forked = true;      // (device-resident batches are produced on the main stream)
    SBR_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    SBR_LAUNCH(launch_build_cells(h->side, h->btgt, h->bsmp, y.Bg, y.S, (int*)h->A(y.a_cells)));
    SBR_LAUNCH(catch_up_rows(h, h->side, kb, sparse_ids(h, kb)));
    SBR_HIP(hipEventRecord(h->ev_cells, h->side));
    h->st.cells_early = true;
    h->side_pending = true;      // (parameters, optimizer state and last[] were written over there: a step abandoned behind
                                 // sbr_forward -- an error return, a ranking, an export -- joins before it reads them)
    return SBR_OK;
}
// the overlapped tail's sort beside the forward chain
static int early_sort(sbr_handle* h) {
    const int rc = tail_sort(h);
    h->st.tail_sorted = true;
    return rc;
}

// one direction: layer l reads the outputs of layer l - 1
static int forward_uni(sbr_handle* h, bool fork_gate) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    for (int l = 0; l < y.L; ++l) {
        const LayerLayout& ly = y.layer[l];
        RecArgs ra = rec_args(h, l);
        if (l == 0) {
            // --r_emb: embeddings of the F indices, flattened, then a dense input projection
            if (y.E) SBR_LAUNCH(launch_gather_concat(s, h->P(y.p_Emb), h->bX, h->A(y.a_emb), y.T, y.Bp, y.F, y.Ep));
            { const int rc = layer0_input(h, ra, ly, h->bX, h->A(y.a_emb)); if (rc != SBR_OK) return rc; }
            mark(h, 1);
        } else {   // dense layers: xt = hid_out(l-1) . W_in + b
            const LayerLayout& lo = y.layer[l - 1];
            SBR_LAUNCH(input_projection(h, ly, h->A(lo.a_hs) + (size_t)y.Bp * lo.Hp, layer_gemm_mode(h, false, false)));
        }
        if (l == 0 && (h->st.tail_sorted || fork_gate)) ra.fence_kb = kTailFenceKb;
        if (fork_gate) { ra.start_word = h->step_words + 128; ra.start_epoch = step_next_epoch(&h->fork_epoch); }
        SBR_LAUNCH_CHAIN(0, s, launch_rec_forward(s, ra, h->plan[l]));
        if (fork_gate) {
            h->st.fork_gated = true; h->step_word_epoch = h->fork_epoch;
            SBR_LAUNCH(launch_step_gate(h->side2, h->step_words + 128, nullptr, h->fork_epoch, (int*)h->A(y.a_fault)));
            { const int rc = early_sort(h); if (rc != SBR_OK) return rc; }
        }
    }
    return SBR_OK;
}

// --r_bi (recurrent_layers.py:70-76).  Level l = forward layer lay.layer[2l] + backwards layer lay.layer[2l+1] over the
// same input.  The backwards layer runs the ordinary kernels on per-row time-reversed copies of its input (see the
// helper kernels in sbr_misc.hip), so every recurrent kernel of the unidirectional path is reused unchanged.
static int forward_bi(sbr_handle* h) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    const int TB = y.T * y.Bp;
    int* Xr = (int*)h->A(y.a_Xr);
    if (!y.E) SBR_LAUNCH(launch_rev_rows_int(s, h->bX, h->blen, Xr, y.T, y.Bp, y.F));
    else {
        SBR_LAUNCH(launch_gather_concat(s, h->P(y.p_Emb), h->bX, h->A(y.a_emb), y.T, y.Bp, y.F, y.Ep));
        SBR_LAUNCH(launch_rev_rows(s, h->A(y.a_emb), h->blen, h->A(y.a_embr), y.T, y.Bp, y.F * y.Ep));
    }
    for (int l = 0; l < y.L; ++l) {
        for (int d = 0; d < 2; ++d) {
            const int pl = 2 * l + d;
            const LayerLayout& ly = y.layer[pl];
            RecArgs ra = rec_args(h, pl);
            if (l == 0) {      // this direction's ids, or its (reversed) flattened embeddings
                const int rc = layer0_input(h, ra, ly, d ? Xr : h->bX, h->A(d ? y.a_embr : y.a_emb)); if (rc != SBR_OK) return rc;
            } else {           // the (reversed) concatenated outputs of the level below
                SBR_LAUNCH(input_projection(h, ly, h->A(d ? y.a_catr[l - 1] : y.a_cat[l - 1]), gemm_mode(h)));
            }
            if (l == 0 && d == 1) mark(h, 1);
            SBR_LAUNCH_CHAIN(0, s, launch_rec_forward(s, ra, h->plan[pl]));
        }
        const LayerLayout& lf = y.layer[2 * l]; const LayerLayout& lb = y.layer[2 * l + 1];
        if (l + 1 < y.L) {
            SBR_LAUNCH(launch_cat_outputs(s, h->A(lf.a_hs), h->A(lb.a_hs), h->blen, h->A(y.a_cat[l]), y.T, y.Bp, lf.Hp));
            SBR_LAUNCH(launch_rev_rows(s, h->A(y.a_cat[l]), h->blen, h->A(y.a_catr[l]), y.T, y.Bp, 2 * lf.Hp));
        } else {   // only_return_final: both directions' last scan output (sparse_lstm.py:485-486)
            SBR_LAUNCH(launch_hcat(s, h->A(lf.a_hs) + (size_t)TB * lf.Hp, h->A(lb.a_hs) + (size_t)TB * lb.Hp, h->A(y.a_hcat), y.Bp, lf.Hp));
        }
    }
    return SBR_OK;
}

extern "C" int sbr_forward(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    if (!h->have_batch) { sbr_set_error("sbr_forward: no batch set"); return SBR_ESTATE; }
    const Layout& y = h->lay; hipStream_t s = h->stream;
    if (sparse_lazy(h))      // the rows this batch gathers must be current before they are read
        for (int b = 0; b < y.n_sparse; ++b)
            if (y.sparse[b].kind == 0)
                SBR_LAUNCH(launch_sparse_catch_up_batch(s, sparse_rows(h, b), sparse_upd(h), h->bX, h->blen, y.T, y.Bp, y.F, (int)h->step_count));
    const bool training = h->st.step_open;
    if (!training) step_reset(h);      // predict, top-k, rank, evaluate (never with the overlapped tail): whatever step was open is discarded
    else { h->st.step_open = false; h->st.tail_nc = h->tail_chunks; h->st.train_fwd_open = true; }      // (step_open: sbr_zero_grads' hand-over, consumed -- a second forward of the step is no training forward)
    // (sbr_build_batch fills the batch set this forward does not read while the step runs: what it needs to know to do that safely)
    h->set_use[h->bb_set] = ++h->batch_seq; h->bb_unread = false;
    bool forked = false;
    if (training) { const int rc = early_cells(h, &forked); if (rc != SBR_OK) return rc; }
    // Overlapped tail, round 3.  Its consumers are throughput-bound once they have the chip's other 192 CUs to themselves (the
    // fence below), so WHEN they start decides when the step ends -- and both waited behind work that does not need the chain:
    // the scatter-add behind the 45 us of the time-chunked sort.  The sort needs nothing but the batch: it runs now, beside the
    // forward chain, for one event record in front of it.  The forward chain claims its CUs' LDS while the sort (118 KB of LDS
    // histogram per workgroup) runs beside it, so the two do not share CUs.
    // Step start without an event (kStepForkGate; single-call step, one layer, one direction, rec_fwd_x6p): the forward chain stores a
    // start word of this step's epoch at its entry, and a one-wave gate on that word stands at the head of the second side stream
    // where the record / wait pair stood -- a word of this epoch means that everything in front of the chain on the main stream is
    // complete and written back, the batch included.  The chain is launched FIRST: a gate is only ever enqueued behind the kernel
    // that releases it, so a forward launch that fails leaves no gate waiting.  
    h->step_word_epoch = 0;
    const bool sort_early = h->st.tail_nc >= 2 && h->sw.tail_overlap == 1;
    const bool fork_gate = kStepForkGate && sort_early && h->in_train_step && y.L == 1 && y.D == 1 && !forked && !step_boundary_marks(h) &&
                           h->plan[0].fwd == REC_X6P;
    if (sort_early && !fork_gate) {
        if (!forked) SBR_HIP(hipEventRecord(h->ev_fork, s));
        SBR_HIP(hipStreamWaitEvent(h->side2, h->ev_fork, 0));
        { const int rc = early_sort(h); if (rc != SBR_OK) return rc; }
    }
    if (training) h->last_fork_gate = fork_gate;
    { const int rc = y.D == 2 ? forward_bi(h) : forward_uni(h, fork_gate); if (rc != SBR_OK) return rc; }
    mark(h, 2);
    h->fwd_done = true;
    return SBR_OK;
}

float* h_last(sbr_handle* h) {   // hid_out[-1] (sparse_lstm.py:485-486) = slot T of the top layer
    const Layout& y = h->lay; const LayerLayout& ly = y.layer[(y.L - 1) * y.D];
    if (y.D == 2) return h->A(y.a_hcat);                 // [forward final | backwards final], filled by forward_bi
    return h->A(ly.a_hs) + (size_t)y.T * y.Bp * ly.Hp;
}

// ---------------------------------------------------------------------------------------
// loss and the output layer's backward
// ---------------------------------------------------------------------------------------
// Work on the side stream that needs only the batch: the sentinel fill of the cluster BPTT kernels' exchange arrays and
// the sort for the embedding scatter-add (the scatter kernel waits for ev_sort).  With cluster kernels it starts now,
// beside the output phase (its own fork event); otherwise it rides behind the ev_lg wait the side stream needs anyway
// -- every event record costs the main stream a few microseconds.
static int side_batch_work(sbr_handle* h, bool fill_needed) {
    const Layout& y = h->lay; hipStream_t sd = h->side;
    if (fill_needed) {
        for (int l = 0; l < y.L * y.D; ++l)
            if (h->plan[l].needs_fill) SBR_LAUNCH(sbr_rec_bwd_cl_fill(sd, rec_args(h, l), h->plan[l].bwd == REC_C16));
        SBR_HIP(hipEventRecord(h->ev_fill, sd)); h->st.fill_done = true;
    }
    // (round 6, call s3: the sort BEHIND the head's record instead of beside the head lets the one-launch sampled head run in 26 us
    // instead of 24 .. 72 by workgroup -- the sort's counting kernels are all atomics -- but beside the BPTT chain it costs the chain
    // more: rec_bwd_c16 375 -> 441 us at C3, 390 -> 404 at C4.  It stays here.)
    if (h->st.tail_nc >= 2) {
        // overlapped tail: the time-chunked sort runs on the SECOND side stream, which consumes it (scatter-add beside the
        // chain); that stream is released by the same record as the first one
        if (h->st.ev_lg_rec) SBR_HIP(hipStreamWaitEvent(h->side2, h->st.ev_lg_rec, 0));      // (NULL: released by the gate -- the sort ran
                                                                                    // beside the forward chain, the consumers wait for the chain's progress words)
        if (!h->st.tail_sorted) { const int rc = tail_sort(h); if (rc != SBR_OK) return rc; }
    } else if (!(y.cfg.flags & SBR_FLAG_ATOMIC_SCATTER) || y.E || y.n_sparse) {
        const SbrSortKeys k = sort_keys(h, 0);
        SBR_LAUNCH(launch_scatter_sort(sd, h->bX, h->blen, y.T, y.Bp, y.F, y.cfg.input_size, k.cnt, k.off, k.cur, k.sid, k.pos,
                                       y.E ? 1 : 0, 0, 1, nullptr, &h->scnt_zero_n));
        if (y.D == 2 && !y.E) {   // the backwards direction scatters with the reversed ids (a_Xr was written by forward_bi)
            const SbrSortKeys k2 = sort_keys(h, 1);
            SBR_LAUNCH(launch_scatter_sort(sd, (const int*)h->A(y.a_Xr), h->blen, y.T, y.Bp, y.F, y.cfg.input_size, k2.cnt, k2.off, k2.cur,
                                           k2.sid, k2.pos, 0));
        }
        SBR_HIP(hipEventRecord(h->ev_sort, sd));
    }
    return SBR_OK;
}

// What releases the side stream once this phase's main-stream work (the head, dh) is enqueued: one record at the end of it,
// which is also the timing mark in front of rec_bwd.  Single-call step with the overlapped tail: no record.  The BPTT chain is
// ordered behind this phase on the main stream and publishes progress words of this step's epoch, so a gate on those words
// at the HEAD of the side stream releases it once the head is complete (tail_gate_wave_kernel, sbr_misc.hip) -- what the
// second side stream does anyway -- and the chain starts without the record's 10 us in front of it.  The
// record stays for phase-by-phase callers, SBR_TAIL_OVERLAP=2, steps without the overlapped tail and a timing mark there.
static int release_side(sbr_handle* h, bool fill_needed) {
    const Layout& y = h->lay; hipStream_t sd = h->side;
    if (kTailGateFirst && h->in_train_step && h->st.tail_nc >= 2 && h->sw.tail_overlap == 1 && h->st.tail_sorted && y.L == 1 && y.D == 1 &&
        !fill_needed && !mark_live(h, 3)) {
        int nwaves = 0;
        int* words = tail_words(h, &nwaves);
        SBR_LAUNCH(launch_tail_gate_wave(sd, words, nwaves, tail_next_epoch(h), y.T, (int*)h->A(y.a_fault)));
        h->st.tail_gated = true;
        // (what sbr_build_batch orders itself behind: sbr_forward's fork -- its record, or the chain's start word where there is none)
        h->ev_step_rec = h->st.fork_gated ? nullptr : h->ev_fork; h->lg_seq = h->batch_seq;      // (no record: st.ev_lg_rec stays NULL)
    } else {
        h->st.ev_lg_rec = h->ev_step_rec = record_shared(h, h->ev_lg, 3); h->lg_seq = h->batch_seq;
        h->step_word_epoch = 0;      // (the record is the later point of the step: the builder takes it)
        SBR_HIP(hipStreamWaitEvent(sd, h->st.ev_lg_rec, 0));
    }
    return SBR_OK;
}

// Round 5: logits, softmax + CCE and dh in ONE launch whose workgroups exchange the row statistics inside the kernel
// (sbr_head.hip; exact-f32 products); its dh leaves as split-K slabs -- folded into the chain's prologue (fold: *keep slabs stay in
// the workspace), or reduced here.  Shapes it does not serve (and SBR_HEAD_FUSE=0) keep the three launches of dense_head_launches.
static int dense_head_fused(sbr_handle* h, bool fold, int* keep, bool* done) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    const int R = h->n_rows, Hp = y.HLt, N = y.N, Nl = (N + 3) & ~3;
    const bool sg = simple_gemm(h), bf16p = (y.cfg.flags & SBR_FLAG_BF16_PROJECTION) && !sg;
    float* ws = h->A(y.a_ws);
    *done = false;
    if (!(h->sw.head_fuse && y.cfg.loss == SBR_LOSS_CCE && !sg && !bf16p && !(y.cfg.flags & SBR_FLAG_F32_MFMA) && y.D == 1 && R == y.Bp))
        return SBR_OK;
    int nsl = 0; hipError_t he = hipSuccess;
    h->head_epoch += 1; if (!h->head_epoch) h->head_epoch = 1;
    if (launch_head_cce(s, h_last(h), h->P(y.p_WoutT), h->P(y.p_bout), h->btgt, h->bpop, h->A(y.a_logits), h->A(y.a_rowcost), ws, y.ws_floats,
                        (unsigned*)h->A(y.a_hstat), (int*)h->A(y.a_fault), y.Bp, N, Nl, Hp, y.Bg, h->head_epoch, h->sw.head_wait_ticks, &nsl, &he,
                        (y.cfg.flags & SBR_FLAG_PROFILE_REC) && (size_t)y.Bp * 16 >= 256 * 8 ? prof_slot(h, 2) : nullptr)) {
        SBR_LAUNCH(he);
        *done = true;
        if (fold) *keep = nsl;
        else SBR_LAUNCH(launch_splitk_reduce(s, ws, nsl, y.Bp, Hp, h->A(y.a_dhlast), Hp, nullptr));
    }
    return SBR_OK;
}
// logits = h . W_out (+ b inside the softmax kernel): DenseLayer (rnn_one_hot.py:65); the loss and dlogits; dh = dlogits . W_out^T
static int dense_head_launches(sbr_handle* h, bool fold, int* keep) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    const int R = h->n_rows, Hp = y.HLt, N = y.N, Nl = (N + 3) & ~3;
    float* lg = h->A(y.a_logits);
    SBR_LAUNCH(launch_gemm(s, projection_mode(h, false), gemm_rowmajor(h_last(h), Hp), gemm_transposed(h->P(y.p_WoutT), Hp), lg, Nl, R, N, Hp));
    if (SBR_LOSS_IS_MARGIN(y.cfg.loss))
        SBR_LAUNCH(launch_margin_loss(s, lg, h->P(y.p_bout), h->btgt, y.NT, h->bX, h->blen, y.T, y.F, h->A(y.a_dflt), h->A(y.a_rowcost), R, N, Nl,
                                      y.Bg, y.cfg.loss, y.cfg.balance, y.cfg.unique));
    else
        SBR_LAUNCH(launch_softmax_cce(s, lg, h->P(y.p_bout), h->btgt, h->bpop, h->A(y.a_rowcost), R, N, Nl, y.Bg));
    SBR_LAUNCH(launch_gemm(s, gemm_mode(h), gemm_rowmajor(lg, Nl), gemm_rowmajor(h->P(y.p_WoutT), Hp), h->A(y.a_dhlast), Hp, R, Hp, N, nullptr,
                           h->A(y.a_ws), y.ws_floats, fold ? keep : nullptr));
    return SBR_OK;
}
// beside the BPTT chain, on the side stream: cost, db_out (+ bias regulariser), dW_out^T [N][Hp] = dlogits^T . h -- and, in a
// single-call step with dense updates, the output layer's step
static int dense_head_grads(sbr_handle* h) {
    const Layout& y = h->lay; hipStream_t sd = h->side;
    const int R = h->n_rows, Hp = y.HLt, N = y.N, Nl = (N + 3) & ~3;
    const bool sg = simple_gemm(h);
    float* lg = h->A(y.a_logits);
    float* hl = h_last(h);
    // Single-call step without a bias regulariser: the output layer's gradient, its step and the batch cost in ONE launch
    // (launch_out_grad_step, sbr_update.hip) instead of the five or six below -- the polling weight-gradient GEMM of the overlapped
    // tail, next on this stream, then starts with the chain instead of 68 us into it.  SBR_OUT_FUSE=0: as before.
    // (taken WITHOUT the overlapped tail only: in front of the polling GEMM of C2 it measured 0.3334 against 0.3294 ms -- that GEMM
    // then starts 9 us earlier and ends where it did, it is throughput-bound beside the chain; C1: 0.3156 -> 0.3035 together with
    // the one-launch head: profiles/round5_variants.txt call b)
    const bool will_step_here = h->in_train_step && !y.n_sparse && !sg && h->st.tail_nc == 0;
    if (h->sw.out_fuse && will_step_here && y.cfg.regularization == 0.0f && y.D == 1) {
        hipError_t oe = hipSuccess;
        if (step_out_grad(h, sd, lg, hl, R, Nl, &oe)) {
            SBR_LAUNCH(oe);
            h->st.out_stepped = true;
        }
    }
    if (!h->st.out_stepped) {
        SBR_LAUNCH(launch_sum_cost(sd, h->A(y.a_rowcost), R, h->cost_ptr()));
        // data-parallel: every rank adds its share of the bias regulariser, shares sum to reg
        const float reg = y.cfg.regularization * (float)R / (float)y.Bg;
        SBR_LAUNCH(launch_colsum_bias(sd, lg, R, N, Nl, h->Gd(y.p_bout), h->P(y.p_bout), reg, h->cost_ptr(), h->A(y.a_csum)));
        SBR_LAUNCH(launch_gemm(sd, gemm_mode(h), gemm_transposed(lg, Nl), gemm_rowmajor(hl, Hp), h->Gd(y.p_WoutT), Hp, N, Hp, R, nullptr,
                               h->A(y.a_ws2), y.ws2_floats));
    }
    SBR_HIP(hipEventRecord(h->ev_og, sd)); h->st.og_recorded = true;   // output-layer gradients + cost complete
    // Single-call step, dense updates: the output layer is stepped right here, beside the BPTT chain (nothing reads W_out
    // any more: dh was computed in front of the record the side stream waited on); sbr_apply_update leaves the range
    // out.  C4: 46 us off the end of the step.  (The overlapped tail does the same itself; phase-by-phase callers --
    // data parallel -- reduce the gradients first.)
    if (h->in_train_step && !y.n_sparse && h->st.tail_nc == 0 && !simple_gemm(h)) {
        if (!h->st.out_stepped) SBR_LAUNCH(step_range(h, sd, y.p_split, y.n_params));
        h->st.out_early = true;
    }
    return SBR_OK;
}
// dense heads: full softmax, or RNNMargin's linear layer
static int loss_dense(sbr_handle* h, bool fill_needed) {
    const Layout& y = h->lay;
    // critical path: dh = dlogits . W_out^T feeds the BPTT chain.  Where the chain is rec_bwd_x6p, the split-K slabs of the dh
    // GEMM stay unreduced and the chain's prologue adds them: one launch (7 us + its gap) less in front of it
    int keep = 0;
    const bool fold = !simple_gemm(h) && y.D == 1 && h->n_rows == y.Bp && h->plan[y.L - 1].bwd == REC_X6P;
    bool head_done = false;
    int rc;
    if ((rc = dense_head_fused(h, fold, &keep, &head_done)) != SBR_OK) return rc;
    if (!head_done && (rc = dense_head_launches(h, fold, &keep)) != SBR_OK) return rc;
    h->st.dh_slabs_n = keep;
    if ((rc = release_side(h, fill_needed)) != SBR_OK) return rc;
    if (!fill_needed && (rc = side_batch_work(h, fill_needed)) != SBR_OK) return rc;
    return dense_head_grads(h);
}

// the cells of a sampled head (targets + samples), and their rows of W_out^T / b_out current
static int sampled_cells(sbr_handle* h) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    int* cells = (int*)h->A(y.a_cells);
    if (h->st.cells_early) SBR_HIP(hipStreamWaitEvent(s, h->ev_cells, 0));      // built and caught up beside the forward chain (sbr_forward)
    else {
        SBR_LAUNCH(launch_build_cells(s, h->btgt, h->bsmp, y.Bg, y.S, cells));
        if (sparse_lazy(h))      // ... and so must the rows of W_out^T / b_out the sampled cells gather
            for (int b = 0; b < y.n_sparse; ++b)
                if (y.sparse[b].kind == 1) SBR_LAUNCH(catch_up_rows(h, s, b, sparse_ids(h, b)));
    }
    h->st.cells_early = false;      // (hand-over from sbr_forward, consumed: a second loss phase of this step builds its cells itself)
    return SBR_OK;
}
// sampled heads (BPR, TOP1, Blackout, ...): the loss over the batch's targets and the shared samples
static int loss_sampled(sbr_handle* h, bool fill_needed) {
    const Layout& y = h->lay; hipStream_t s = h->stream, sd = h->side;
    const int R = h->n_rows, Hp = y.HLt, C = y.C;
    float* hl = h_last(h);
    int* cells = (int*)h->A(y.a_cells);
    float *Wc = h->A(y.a_Wc), *bc = h->A(y.a_bc), *act = h->A(y.a_act), *dWc = h->A(y.a_dWc), *dbc = h->A(y.a_dbc);
    { const int rc = sampled_cells(h); if (rc != SBR_OK) return rc; }
    SBR_LAUNCH(launch_gather_rows(s, h->P(y.p_WoutT), h->P(y.p_bout), cells, C, Hp, Wc, bc));
    // Round 6: activations, loss, its gradient and dh in ONE launch where the shape allows it (head_sampled_kernel, sbr_head.hip):
    // four launches on twenty workgroups each were 113 us between the two chains of C3.  SBR_HEAD_FUSE=0: the launches below.
    bool head1 = false;
    if (head_sampled_taken(h, R)) {
        hipError_t he = hipSuccess;
        head1 = launch_head_sampled(s, hl, Wc, bc, h->bpop, act, h->A(y.a_rowcost), h->A(y.a_dhlast), R, C, Hp, y.Bg, y.S,
                                    y.cfg.row_offset, y.cfg.loss, y.Bg, &he,
                                    (y.cfg.flags & SBR_FLAG_PROFILE_REC) ? prof_slot(h, 2) : nullptr);
        if (head1) SBR_LAUNCH(he);
    }
    if (!head1) {
        SBR_LAUNCH(launch_gemm(s, gemm_mode(h), gemm_rowmajor(hl, Hp), gemm_transposed(Wc, Hp), act, C, R, C, Hp));
        SBR_LAUNCH(launch_sampled_loss(s, act, bc, h->bpop, h->A(y.a_rowcost), R, y.Bg, y.S, y.cfg.row_offset,
                                       y.cfg.loss, y.Bg));
    }
    // Round 5: dh feeds the BPTT chain, everything else here only feeds the optimizer -- cost sum, bias column sums, the dWc GEMM
    // and the scatter of the cells' gradients (5 launches, ~75 us at C3 beside the side stream's sort) leave the main stream: dh
    // first, one record, the rest on the side stream beside the chain (as the dense heads always did).
    if (!head1) SBR_LAUNCH(launch_gemm(s, gemm_mode(h), gemm_rowmajor(act, C), gemm_rowmajor(Wc, Hp), h->A(y.a_dhlast), Hp, R, Hp, C));
    { const int rc = release_side(h, fill_needed); if (rc != SBR_OK) return rc; }
    SBR_LAUNCH(launch_sum_cost(sd, h->A(y.a_rowcost), R, h->cost_ptr()));
    SBR_LAUNCH(launch_colsum_bias(sd, act, R, C, C, dbc, nullptr, 0.0f, nullptr, h->A(y.a_csum)));
    SBR_LAUNCH(launch_gemm(sd, gemm_mode(h), gemm_transposed(act, C), gemm_rowmajor(hl, Hp), dWc, Hp, C, Hp, R));
    SBR_LAUNCH(launch_scatter_cells(sd, h->Gd(y.p_WoutT), h->Gd(y.p_bout), dWc, dbc, cells, C, Hp));
    SBR_HIP(hipEventRecord(h->ev_og, sd)); h->st.og_recorded = true;
    if (!fill_needed) {      // the batch-only side work follows (the side stream has waited for this phase's record)
        const int rc = side_batch_work(h, fill_needed); if (rc != SBR_OK) return rc;
    }
    // Single-call step: the head's row-sparse block (W_out^T rows + b_out of the sampled cells) has its complete gradient now
    // and nothing reads those rows any more (dh is computed): its step runs on the side stream beside the BPTT chain instead
    // of at the end of the step (C3: 35 us, C5: 41 us); sbr_apply_update leaves the block out.
    if (h->in_train_step && h->sw.sparse_out_early)
        for (int b = 0; b < y.n_sparse; ++b)
            if (y.sparse[b].kind == 1 && !h->st.sp_exchanged[b]) {
                SBR_HIP(hipStreamWaitEvent(sd, h->ev_og, 0));      // (recorded on this very stream)
                SBR_LAUNCH(step_rows(h, sd, b, sparse_ids(h, b)));
                h->st.wout_early = true;
            }
    return SBR_OK;
}

extern "C" int sbr_loss_backward_output(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    if (!h->fwd_done) { sbr_set_error("sbr_loss_backward_output: call sbr_forward first"); return SBR_ESTATE; }
    const Layout& y = h->lay; hipStream_t s = h->stream, sd = h->side;
    h->grads_clean = false;
    // (the output layer's input is Bp rows of HLt floats: both directions with --r_bi)
    if (h->n_rows < y.Bp) SBR_HIP(hipMemsetAsync(h->A(y.a_dhlast), 0, (size_t)y.Bp * y.HLt * sizeof(float), s));   // padded rows carry no gradient
    h->side_pending = true;
    h->last_tail_gated = 0;
    h->last_join_gate = 0;
    // the batch-only side work (side_batch_work): beside the head where the cluster BPTT kernels need their sentinel fill, else behind it
    bool fill_needed = false;
    for (int l = 0; l < y.L * y.D; ++l) fill_needed = fill_needed || h->plan[l].needs_fill;
    if (fill_needed) {
        SBR_HIP(hipEventRecord(h->ev_fork, s));
        SBR_HIP(hipStreamWaitEvent(sd, h->ev_fork, 0));
        const int rc = side_batch_work(h, fill_needed); if (rc != SBR_OK) return rc;
    }
    const bool dense = y.cfg.loss == SBR_LOSS_CCE || SBR_LOSS_IS_MARGIN(y.cfg.loss);
    { const int rc = dense ? loss_dense(h, fill_needed) : loss_sampled(h, fill_needed); if (rc != SBR_OK) return rc; }
    mark(h, 3);
    if (h->deferred_join && !h->in_train_step) {
        // the caller orders its collective behind the SIDE stream: make that stream also cover what this phase wrote
        // to the output-layer gradients on the main stream (sampled heads)
        SBR_HIP(hipEventRecord(h->ev_lg, s));
        SBR_HIP(hipStreamWaitEvent(sd, h->ev_lg, 0));
        return SBR_OK;
    }
    // called on its own (the caller reads the output-layer gradients next): join now
    if (!h->in_train_step) return side_join(h);
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// backward through the recurrent layers
// ---------------------------------------------------------------------------------------
// the BPTT kernel's arguments for layer pl whose gradient from above is dh_last (top level) or its own a_dhext
static int bptt_args(sbr_handle* h, int pl, const float* dh_last, bool wait_fill, RecArgs* out) {
    const Layout& y = h->lay; const LayerLayout& ly = y.layer[pl];
    RecArgs a = rec_args(h, pl);
    if (h->st.fill_done && h->plan[pl].needs_fill) {
        a.sentinel_done = 1;
        if (wait_fill) SBR_HIP(hipStreamWaitEvent(h->stream, h->ev_fill, 0));
    }
    a.dh_last = dh_last;
    a.dh_ext = pl / y.D < y.L - 1 ? h->A(ly.a_dhext) : nullptr;
    *out = a;
    return SBR_OK;
}

// How a layer's dW_hid is computed beside (or behind) its BPTT chain
struct WgradPlan {
    int nc;             // BPTT launches (time chunks)
    int nsl;            // K-slices (= workgroups of the wgrad kernel) per chunk
    size_t slab;        // floats of one dW_hid partial
    bool side;          // weight gradients on the side stream
    bool gemm;          // ... by the bf16x6 GEMM (else the dedicated f32 kernel)
    bool f16;           // ... on fp16 x3 products
    bool swap;          // the main stream keeps the weight-gradient branch, the side stream takes partials + scatter
};
static WgradPlan wgrad_plan(const sbr_handle* h, const LayerLayout& ly, const RecArgs& a) {
    const Layout& y = h->lay;
    const int GHp = y.G * ly.Hp;
    const bool sg = simple_gemm(h);
    WgradPlan p;
    // BPTT in time chunks when the bf16x6 kernel runs: dW_hid of a finished chunk is computed on the side
    // stream (190 idle CUs) while the chain continues
    p.slab = (size_t)ly.Hp * GHp;
    p.nc = (plan_of(h, ly).bwd_chunkable && y.T >= 64 && !sg) ? h->sw.bwd_chunks : 1;
    p.nsl = (int)std::min<size_t>(kWgradSlices / p.nc, y.ws2_floats / (p.slab * p.nc));   // K-slices (= workgroups of the wgrad kernel)
    if (p.nsl < 1) p.nc = 1;
    p.side = !simple_rec(h) && !sg && p.nsl >= 1;   // weight gradients on the side stream
    // the bf16x6 GEMM covers the slab with 128x128 tiles: ~512 workgroups in all is enough (the dedicated f32
    // kernel, one workgroup per slab, wants many thin slabs)
    p.gemm = (!(y.cfg.flags & SBR_FLAG_F32_MFMA) && ly.Hp >= 96) || !(ly.Hp == 32 || ly.Hp == 64 || ly.Hp == 128);
    // fp16 x3 products for that GEMM: its operands are hidden states (|h| <= 1 behind tanh / sigmoid gates) and gradients
    // that have passed the clip at +-100 (scaled by 2^9 into fp16's range), see gemm_x6_kernel NP = 2
    p.f16 = h->sw.wgrad_f16 && !a.relu && y.cfg.grad_clip > 0.0f && y.cfg.grad_clip <= 100.0f;
    if (p.gemm && p.nsl > 1) {
        p.nsl = std::max(1, std::min(p.nsl, kWgradX6Wgs / (((ly.Hp + 127) / 128) * ((GHp + 127) / 128)) / p.nc));
    }
    // Tail of a single-layer step with one BPTT launch: the main stream keeps the longer branch (dW_hid GEMM + slab
    // reduction + its updates) and the side stream takes the bias partials, the embedding scatter-add and their
    // updates -- the main stream then ends the step without waiting ~13 us for a cross-stream event behind the
    // branch that finishes last (profiles/round1_i_timeline.txt).
    p.swap = p.side && p.nc == 1 && y.L == 1 && !y.E && !y.n_sparse &&
             y.n_params <= ((size_t)4 << 20) &&      // large models (C4: 34 M parameters) measured 2 % slower this way
             !(y.cfg.flags & SBR_FLAG_ATOMIC_SCATTER);   // phase-by-phase callers (data parallel) join the side stream
                                                         // before their collective: same split of the tail
    return p;
}

// the K-slab table of the overlapped tail's polling GEMM: built and uploaded on the first step of a shape
static int tail_slab_table(sbr_handle* h, int K, int cap, SbrPoll* pl) {
    if (h->tail_slab_key[0] != K || h->tail_slab_key[1] != cap || !h->tail_slab_dev) {      // (first step of this shape)
        sbr_tail_slab_table(K, h->lay.Bp, 255, kTailSlabGrowth, kTailSlabMax, h->tail_slab_host);
        if (!h->tail_slab_dev) SBR_HIP(hipMalloc(&h->tail_slab_dev, 260 * sizeof(int)));
        SBR_HIP(hipMemcpy(h->tail_slab_dev, h->tail_slab_host.data(), h->tail_slab_host.size() * sizeof(int), hipMemcpyHostToDevice));
        h->tail_slab_key[0] = K; h->tail_slab_key[1] = cap;
    }
    pl->slab_lo = h->tail_slab_dev;
    pl->n_slabs = (int)h->tail_slab_host.size() - 1;
    return SBR_OK;
}

// ---- Overlapped tail.  The chain (64 of 256 CUs at C2) stores dxt / dhi write-through and every wave publishes the
// time step it has completed.  Two consumers run beside it on the idle CUs, ONE launch each, whose workgroups /
// waves wait inside the kernel for the time steps they read (SbrPoll, sbr_common.h):
//   side stream   (the output layer's gradient kernels, left over from the loss phase ->) gate (returns once every wave
//                 of the chain has published: the chain is resident, spinning consumers can no longer keep it off the
//                 chip) -> dW_hid GEMM: persistent groups of workgroups share the K slabs of a table in the order the
//                 chain releases them, one partial each -> reduction of the partials (-> W_hid update)
//   second side   (the time-chunked sort and the ids' running cost, beside the FORWARD chain ->) the same gate ->
//   stream        embedding scatter-add: units that own id ranges of equal cost add their rows in LDS and store each
//                 once; workgroup 0 of that launch is the MONITOR, which folds the chain's progress words into the
//                 word every consumer polls (-> W_in update)
//   main stream   chain -> bias / init-state partial sums (-> their update) -> joins both
// In a single-call step every stream applies the optimizer to what it has produced (the output layer early, on
// the side stream); phase-by-phase callers (data parallel) get complete gradients and update in sbr_apply_update.
// Layer 0 of a one-layer step whose forward planned the tail (h->st.tail_nc >= 2); the whole of the layer's backward.
static int backward_tail(sbr_handle* h, RecArgs& a, const WgradPlan& wp, int nblk) {
    const Layout& y = h->lay; const LayerLayout& ly = y.layer[0];
    hipStream_t s = h->stream, sd = h->side;
    const int GHp = y.G * ly.Hp;
    const size_t slab = wp.slab;
    float* ws2 = h->A(y.a_ws2);
    const int tnc = h->st.tail_nc;
    // SBR_TAIL_OVERLAP=2: the same kernels, all on the main stream behind the chain (nothing has to run concurrently):
    // for tools that serialise kernels (rocprofv3 --pmc) and for triage
    const bool serial = h->sw.tail_overlap == 2;
    hipStream_t s2 = serial ? s : h->side2;
    if (serial) {
        sd = s;
        { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
        SBR_HIP(hipEventRecord(h->ev_tail2, h->side2));           // the sort ran there
        SBR_HIP(hipStreamWaitEvent(s, h->ev_tail2, 0));
    }
    const bool gru = y.cfg.cell == SBR_CELL_GRU;
    int nwaves = 0;
    int* words = tail_words(h, &nwaves);
    int* done = (int*)h->A(y.a_done);
    // (the side stream's gate of this step may already wait for the epoch: sbr_loss_backward_output)
    const bool gated = h->st.tail_gated && !serial;
    h->st.tail_gated = false; h->last_tail_gated = gated;      // (hand-over from the loss phase, consumed: the gate waits for ONE chain, this one)
    a.progress = words; a.prog_every = kTailPubEvery; a.prog_epoch = gated ? h->prog_epoch : tail_next_epoch(h);
    const int K = y.T * y.Bp;
    const int cap = (int)std::min<size_t>(256, y.ws2_floats / slab);
    SbrPoll pl{words, nwaves, done, a.prog_epoch, y.Bp, a.fault, 0, 0, h->tail_trace, nullptr, 0};
    { const int rc = tail_slab_table(h, K, cap, &pl); if (rc != SBR_OK) return rc; }
    const int n_slabs = std::max(1, std::min(std::min(kTailGemmGroups, cap), pl.n_slabs));      // partials = persistent groups
    const bool upd_here = h->in_train_step;
    if (!serial) a.fence_kb = kTailFenceKb;              // the chain's CUs are its own: the consumers take the other 192
    SBR_LAUNCH_CHAIN(1, s, launch_rec_backward(s, a, h->plan[0]));
    mark(h, 4);
    // side stream: output layer first (its gradients are complete on this stream: dW_out GEMM, bias sums)
    const bool out_early = upd_here && (y.cfg.loss == SBR_LOSS_CCE || SBR_LOSS_IS_MARGIN(y.cfg.loss));
    if (out_early && !h->st.out_stepped)       // (else: launch_out_grad_step has stepped the output layer with its gradient, sbr_loss_backward_output)
        SBR_LAUNCH(step_range(h, sd, y.p_split, y.n_params));
    // the monitor: on a stream of its own behind nothing but the chain's first progress words (its own loop waits for them)
    // ... unless the scatter-add launch carries it (default where that launch is the LDS-row one and has its own stream)
    const bool mon_in_units = !serial && h->scat.tail == SCAT_LDS;
    if (!mon_in_units) SBR_LAUNCH(launch_tail_monitor(serial ? s : h->side3, pl, a.t_lo));
    if (!gated) SBR_LAUNCH(launch_tail_gate(sd, words, nwaves, a.prog_epoch, y.T, a.fault));      // (else: at the head of this stream)
    {
        hipError_t we = hipSuccess;
        if (!launch_gemm_slabs_x6_poll(sd, wgrad_gemm_mode(h, wp.f16), gemm_transposed(h->A(ly.a_hs), ly.Hp), gemm_rowmajor(a.dxt, GHp), ly.Hp,
                                       GHp, K, ws2, n_slabs, GHp, slab, gru ? a.dhi : nullptr, ly.Hp, gru ? 2 * ly.Hp : 0, &we, pl)) {
            sbr_set_error("overlapped tail: the weight-gradient GEMM rejected the shape"); return SBR_EINVAL;
        }
        SBR_LAUNCH(we);
    }
    // (the second side stream: behind the record where there is one; without it this gate is on the chip from the sort's
    // end on, beside the forward chain and the head -- the one-wave form there too)
    if (gated) SBR_LAUNCH(launch_tail_gate_wave(s2, words, nwaves, a.prog_epoch, y.T, a.fault));
    else if (!serial) SBR_LAUNCH(launch_tail_gate(s2, words, nwaves, a.prog_epoch, y.T, a.fault));
    // (tried and dropped: the last time chunk as a launch of its own behind the polling one, one wave per 16 entries on the
    // then idle chip -- the hot rows' atomics serialise there: 23 us for 6400 entries, profiles/round3_variants.txt call d)
    const SbrSortKeys k = sort_keys(h, 0);
    h->last_scatter_form = h->scat.tail;
    if (h->scat.tail == SCAT_LDS)
        SBR_LAUNCH(launch_scatter_lds_poll(s2, h->Gd(ly.p_Win), a.dxt, k.sid, k.pos, k.off, (const int*)h->A(y.a_sP), y.cfg.input_size, tnc,
                                           GHp, pl, h->tail_bounds, kTailScatterUnits, h->scat, mon_in_units, a.t_lo));
    else
        SBR_LAUNCH(launch_scatter_reduce_poll(s2, h->Gd(ly.p_Win), a.dxt, k.sid, k.pos, k.off, y.cfg.input_size, tnc, sort_entries(y),
                                              GHp, y.Bp, pl, h->tail_bounds, kTailShortChunks, !serial && kTailFenceKb > 0, h->scat));
    // Step end without an event wait (kStepJoinGate; single-call step): behind the last kernel of either consumer stream a
    // one-lane kernel stores a completion word of this step's epoch at its entry (kernel to kernel on one queue: no gap), and
    // ONE gate on both words, behind this stream's own last kernel, is the join.  The events are still recorded on their
    // streams (sbr_join_side, the data-parallel driver and callers that restore or read parameters from another stream use
    // them).  DESIGN.md section 3f.
    const bool join_gate = kStepJoinGate && upd_here && !serial && !step_boundary_marks(h);
    if (join_gate) step_next_epoch(&h->join_epoch);
    h->last_join_gate = join_gate;
    if (upd_here) SBR_LAUNCH(step_range(h, s2, ly.p_Win, ly.p_b));
    if (join_gate) SBR_LAUNCH(launch_step_word(s2, h->step_words + 96, h->join_epoch));
    SBR_HIP(hipEventRecord(h->ev_tail2, s2));
    // single-call step: the slab reduction IS the W_hid update (one launch, one pass less behind the chain); phase-by-phase
    // callers (data parallel) need the reduced gradient
    if (upd_here && ly.p_peep - ly.p_Whid == slab && (slab & 3) == 0) {
        SBR_LAUNCH(step_from_slabs(h, sd, ws2, n_slabs, ly.p_Whid, slab));
    } else {
        SBR_LAUNCH(launch_splitk_reduce(sd, ws2, n_slabs, ly.Hp, GHp, h->Gd(ly.p_Whid), GHp, nullptr));
        if (upd_here) SBR_LAUNCH(step_range(h, sd, ly.p_Whid, ly.p_peep));
    }
    if (join_gate) SBR_LAUNCH(launch_step_word(sd, h->step_words + 32, h->join_epoch));
    SBR_HIP(hipEventRecord(h->ev_tail, sd));
    // main stream, behind the chain
    SBR_LAUNCH(reduce_partials(h, s, ly, a, nblk));
    mark(h, 5);
    if (upd_here) {      // b, then (behind the gap that is W_hid) peepholes / initial states, and the output layer unless done
        // (a sampled head's gradient kernels run on the side stream since round 5, and this launch reads
        // and clears their output: order it behind them.  Without the wait the chain's length hid the race.)
        if (!out_early && h->st.og_recorded) SBR_HIP(hipStreamWaitEvent(s, h->ev_og, 0));
        SBR_LAUNCH(step_range(h, s, ly.p_b, out_early ? y.p_split : y.n_params, ly.p_Whid - ly.p_b, ly.p_peep - ly.p_Whid));
        h->st.tail_updated = true;
    }
    if (h->deferred_join && !h->in_train_step && !serial) {
        // data-parallel driver: it orders one collective behind each producing stream (W_in: second side stream,
        // W_hid: side stream, the rest: this stream) and joins through sbr_join_side / sbr_apply_update
        h->tail_join_pending = true;
        mark(h, 6);
        return SBR_OK;
    }
    if (join_gate) {      // (no mark 6 here: step_boundary_marks)
        SBR_LAUNCH(launch_step_gate(s, h->step_words + 32, h->step_words + 96, h->join_epoch, a.fault));
        h->side_pending = false;
        return SBR_OK;
    }
    SBR_HIP(hipStreamWaitEvent(s, h->ev_tail2, 0));
    mark(h, 6);
    SBR_HIP(hipStreamWaitEvent(s, h->ev_tail, 0));
    h->side_pending = false;
    return SBR_OK;
}

// BPTT of layer l in wp.nc launches; dW_hid of each finished chunk on stream sw beside the rest of the chain, the partial sums on sm
static int backward_chunked(sbr_handle* h, int l, RecArgs& a, const WgradPlan& wp, int nblk, hipStream_t sw, hipStream_t sm) {
    const Layout& y = h->lay; const LayerLayout& ly = y.layer[l];
    hipStream_t s = h->stream, sd = h->side;
    const int GHp = y.G * ly.Hp, nc = wp.nc, nsl = wp.nsl;
    const size_t slab = wp.slab;
    float* ws2 = h->A(y.a_ws2);
    for (int c = 0; c < nc; ++c) {
        a.t_hi = (int)((long)y.T * (nc - c) / nc); a.t_lo = (int)((long)y.T * (nc - c - 1) / nc); a.chunk = c;
        SBR_LAUNCH_CHAIN(1, s, launch_rec_backward(s, a, h->plan[l]));
        // (this layer's main-stream record behind the BPTT launch)
        hipEvent_t ev_chain_end = record_shared(h, h->ev_chunk[c], (l == 0 && c == nc - 1) ? 4 : -1);
        SBR_HIP(hipStreamWaitEvent(sd, ev_chain_end, 0));
        // dW_hid [Hp][G*Hp] += hs[t]^T . dhi[t] over the chunk's positions (hs slot t = h_{t-1})
        const float* hsc = h->A(ly.a_hs) + (size_t)a.t_lo * y.Bp * ly.Hp;
        const GemmOperand hsT = gemm_transposed(hsc, ly.Hp);
        const int Kc = (a.t_hi - a.t_lo) * y.Bp;
        float* slabs = ws2 + (size_t)c * nsl * slab;
        const bool gru = y.cfg.cell == SBR_CELL_GRU;
        const float* dxc = a.dxt + (size_t)a.t_lo * y.Bp * GHp;
        const float* dhcc = gru ? a.dhi + (size_t)a.t_lo * y.Bp * ly.Hp : nullptr;
        hipError_t we = hipSuccess;
        // swapped tail: this GEMM's slabs share the second workspace with the split-K slabs of the side stream's dW_out
        // GEMM -- normally long reduced by now, but nothing ordered the two (a wait on a complete event is free)
        if (sw == s && h->st.og_recorded) SBR_HIP(hipStreamWaitEvent(s, h->ev_og, 0));
        if (!wp.gemm && launch_wgrad_slabs(sw, hsc, dxc, dhcc, slabs, ly.Hp, GHp, Kc, nsl, &we)) {
            SBR_LAUNCH(we);
        } else if (launch_gemm_slabs_x6(sw, wgrad_gemm_mode(h, wp.f16), hsT, gemm_rowmajor(dxc, GHp), ly.Hp, GHp, Kc, slabs, nsl, GHp, slab,
                                        dhcc, ly.Hp, gru ? 2 * ly.Hp : 0, &we)) {
            SBR_LAUNCH(we);     // one bf16x6 GEMM: columns [0, 2Hp) from dxt, the candidate-gate columns from the compact array
        } else if (gru) {   // hid_input grad = [dxt_r | dxt_u | dhi_c]
            SBR_LAUNCH(launch_gemm_slabs(sw, gemm_mode(h), hsT, gemm_rowmajor(dxc, GHp), ly.Hp, 2 * ly.Hp, Kc, slabs, nsl, GHp, slab));
            SBR_LAUNCH(launch_gemm_slabs(sw, gemm_mode(h), hsT, gemm_rowmajor(dhcc, ly.Hp), ly.Hp, ly.Hp, Kc, slabs + 2 * ly.Hp, nsl, GHp, slab));
        } else {
            SBR_LAUNCH(launch_gemm_slabs(sw, gemm_mode(h), hsT, gemm_rowmajor(dxc, GHp), ly.Hp, GHp, Kc, slabs, nsl, GHp, slab));
        }
    }
    SBR_LAUNCH(launch_splitk_reduce(sw, ws2, nc * nsl, ly.Hp, GHp, h->Gd(ly.p_Whid), GHp, nullptr));
    h->side_pending = true;
    if (l == 0) mark(h, 4);
    if (wp.swap) h->st.tail_swapped = true;
    SBR_LAUNCH(reduce_partials(h, sm, ly, a, nc * nblk));
    return SBR_OK;
}

// The gradient of the index-input rows of layer 0 (direction dir: layer ly, its dxt) in the form h->scat.plain, on stream st: per-element
// atomics over the ids themselves, or one of the forms over the plain-key sort of that direction's ids.  The one launch site of these
// forms: the step (layer0_scatter, backward_bi) and sbr_debug_scatter.
static int scatter_plain(sbr_handle* h, hipStream_t st, int dir, const LayerLayout& ly, const float* dxt) {
    const Layout& y = h->lay; const ScatPlan& p = h->scat;
    const int GHp = y.G * ly.Hp, n_ids = y.cfg.input_size;
    float* dW = h->Gd(ly.p_Win);
    const SbrSortKeys k = sort_keys(h, dir);
    float* part = h->A(y.a_srpart); int* aux = (int*)h->A(y.a_srid);
    if (p.plain == SCAT_ATOMIC) SBR_LAUNCH(launch_scatter_rows(st, dW, dxt, dir ? (const int*)h->A(y.a_Xr) : h->bX, h->blen, y.T, y.Bp, y.F, GHp));
    else if (p.plain == SCAT_RANGE) SBR_LAUNCH(launch_scatter_range(st, dW, dxt, k.sid, k.pos, k.off, n_ids, GHp, part, aux, SBR_SCAT_RANGES, p));
    else if (p.plain == SCAT_WIDE) SBR_LAUNCH(launch_scatter_wide(st, dW, dxt, k.sid, k.pos, k.off, n_ids, sort_entries(y), GHp, part, aux, y.sr_slots, p));
    else SBR_LAUNCH(launch_scatter_reduce(st, dW, dxt, k.sid, k.pos, k.off, n_ids, sort_entries(y), GHp, y.Bp, p.reduce));
    return SBR_OK;
}
// ... of a one-direction step: the sorted forms on stream sm (the atomics stay on the main stream); sbr_query "scatter_form"
static int layer0_scatter(sbr_handle* h, const RecArgs& a, hipStream_t sm) {
    hipStream_t s = h->stream;
    const bool sorted = h->scat.plain != SCAT_ATOMIC;
    if (sorted && sm == s) SBR_HIP(hipStreamWaitEvent(s, h->ev_sort, 0));      // (the sort ran on the side stream)
    h->last_scatter_form = h->scat.plain;
    return scatter_plain(h, sorted ? sm : s, 0, h->lay.layer[0], a.dxt);
}

// the stand-alone scatter-add of layer 0's embedding gradient over the current batch, timed on its own (include/sbr_rnn.h)
extern "C" int sbr_debug_scatter(sbr_handle* h, int reps, float* us, int64_t* entries, int64_t* rows) {
    CHECK_ARG(h && us && reps >= 1 && reps <= 1000, "bad argument");
    const Layout& y = h->lay;
    if (!h->have_batch || y.E || y.D != 1) { sbr_set_error("sbr_debug_scatter: needs a batch and an index-input, one-direction layer 0"); return SBR_ESTATE; }
    const LayerLayout& ly = y.layer[0];
    const int GHp = y.G * ly.Hp;
    hipStream_t s = h->stream;
    SBR_HIP(hipDeviceSynchronize());                      // nothing beside it
    const SbrSortKeys k = sort_keys(h, 0);
    SBR_LAUNCH(launch_scatter_sort(s, h->bX, h->blen, y.T, y.Bp, y.F, y.cfg.input_size, k.cnt, k.off, k.cur, k.sid, k.pos, 0, 0, 1, nullptr,
                                   &h->scnt_zero_n));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    SBR_HIP(hipEventCreate(&e0)); SBR_HIP(hipEventCreate(&e1));
    const float* dxt = h->A(ly.a_dxt);
    auto one = [&]() { return scatter_plain(h, s, 0, ly, dxt); };      // the step's own launch (layer0_scatter)
    for (int i = 0; i < 2; ++i) { const int rc = one(); if (rc != SBR_OK) return rc; }
    SBR_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < reps; ++i) { const int rc = one(); if (rc != SBR_OK) return rc; }
    SBR_HIP(hipEventRecord(e1, s));
    SBR_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SBR_HIP(hipEventElapsedTime(&ms, e0, e1));
    *us = ms * 1000.0f / (float)reps;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (entries || rows) {
        std::vector<int> off((size_t)y.cfg.input_size + 1);
        SBR_HIP(hipMemcpy(off.data(), k.off, off.size() * sizeof(int), hipMemcpyDeviceToHost));
        int64_t nr = 0;
        for (int i = 0; i < y.cfg.input_size; ++i) nr += off[i + 1] > off[i];
        if (entries) *entries = off[y.cfg.input_size];
        if (rows) *rows = nr;
    }
    // the gradient block as a step expects it: zero (the rows the scatter-add wrote, i.e. the whole block)
    SBR_HIP(hipMemsetAsync(h->Gd(ly.p_Win), 0, (size_t)y.cfg.input_size * GHp * sizeof(float), s));
    SBR_HIP(hipStreamSynchronize(s));
    h->st.tail_sorted = false;      // (no reset: called between a forward and its loss phase, the step goes on -- without the time-chunked keys this call's sort overwrote)
    return SBR_OK;
}

// layer l of the one-direction road: its BPTT chain, its weight gradients and the gradient wrt its input
static int backward_layer(sbr_handle* h, int l) {
    const Layout& y = h->lay; hipStream_t s = h->stream, sd = h->side;
    const LayerLayout& ly = y.layer[l];
    const bool top = l == y.L - 1;
    RecArgs a;
    { const int rc = bptt_args(h, l, top ? h->A(y.a_dhlast) : nullptr, top, &a); if (rc != SBR_OK) return rc; }
    if (top && h->st.dh_slabs_n > 0) { a.dh_slabs = h->A(y.a_ws); a.n_dh_slabs = h->st.dh_slabs_n; }      // (sbr_loss_backward_output)
    if (a.prof) a.prof = prof_slot(h, 1);
    const int nblk = h->plan[l].bwd_blocks;
    const WgradPlan wp = wgrad_plan(h, ly, a);
    if (l == 0 && y.L == 1 && h->st.tail_nc >= 2) return backward_tail(h, a, wp, nblk);      // the whole of the layer
    hipStream_t sw = wp.swap ? s : sd;      // weight-gradient GEMM
    hipStream_t sm = wp.swap ? sd : s;      // partials + scatter
    if (wp.nc > 1 || wp.side) {
        const int rc = backward_chunked(h, l, a, wp, nblk, sw, sm); if (rc != SBR_OK) return rc;
    } else {
        SBR_LAUNCH_CHAIN(1, s, launch_rec_backward(s, a, h->plan[l]));
        if (l == 0) mark(h, 4);
        SBR_LAUNCH(reduce_partials(h, s, ly, a, nblk));
        { const int rc = whid_grad_gemm(h, ly, a); if (rc != SBR_OK) return rc; }
    }
    if (l == 0 && y.E) {
        mark(h, 5);
        // dense layer 0 behind the embedding: dW_in = emb^T . dxt, d_emb = dxt . W_in^T, then the scatter-add into dW_emb
        int rc;
        if ((rc = input_grads_dense(h, ly, a, h->A(y.a_emb), h->A(y.a_demb), false)) != SBR_OK) return rc;
        if ((rc = emb_grad_scatter(h)) != SBR_OK) return rc;
        mark(h, 6);
    } else if (l == 0) {
        mark_on(h, 5, sm);
        { const int rc = layer0_scatter(h, a, sm); if (rc != SBR_OK) return rc; }
        mark_on(h, 6, sm);
    } else {      // dW_in = h^{l-1 T} . dxt, dh^{l-1} = dxt . W_in^T
        const LayerLayout& lo = y.layer[l - 1];
        const float* xin = h->A(lo.a_hs) + (size_t)y.Bp * lo.Hp;     // input at step t = h^{l-1}_t = slot t+1
        return input_grads_dense(h, ly, a, xin, h->A(lo.a_dhext), true);
    }
    return SBR_OK;
}
// one direction, top layer first
static int backward_uni(sbr_handle* h) {
    for (int l = h->lay.L - 1; l >= 0; --l) { const int rc = backward_layer(h, l); if (rc != SBR_OK) return rc; }
    if (!h->in_train_step && !h->deferred_join) return side_join(h);
    return SBR_OK;
}

// --r_bi: per level the forward layer, then the backwards layer (whose arrays are in reversed time)
static int backward_bi(sbr_handle* h) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    SBR_LAUNCH(launch_split_cols(s, h->A(y.a_dhlast), h->A(y.a_dhl[0]), h->A(y.a_dhl[1]), y.Bp, y.HLp));
    for (int l = y.L - 1; l >= 0; --l) {
        for (int d = 0; d < 2; ++d) {
            const int pl = 2 * l + d;
            const LayerLayout& ly = y.layer[pl];
            RecArgs a;
            { const int rc = bptt_args(h, pl, l == y.L - 1 ? h->A(y.a_dhl[d]) : nullptr, true, &a); if (rc != SBR_OK) return rc; }
            const int nblk = h->plan[pl].bwd_blocks;
            SBR_LAUNCH_CHAIN(1, s, launch_rec_backward(s, a, h->plan[pl]));
            if (l == 0 && d == 1) mark(h, 4);
            SBR_LAUNCH(reduce_partials(h, s, ly, a, nblk));
            { const int rc = whid_grad_gemm(h, ly, a); if (rc != SBR_OK) return rc; }
            if (l == 0 && !y.E) {   // index input: scatter-add with this direction's ids (the backwards one sorted its reversed ids)
                if (d == 0) mark(h, 5);
                // (two directions: the plan says form 0 -- each with its own sort -- or the atomics; "scatter_form" is not set here)
                if (h->scat.plain != SCAT_ATOMIC) SBR_HIP(hipStreamWaitEvent(s, h->ev_sort, 0));
                { const int rc = scatter_plain(h, s, d, ly, a.dxt); if (rc != SBR_OK) return rc; }
            } else {                // dense input, in this direction's time order
                const float* inp = l == 0 ? h->A(d ? y.a_embr : y.a_emb) : h->A(d ? y.a_catr[l - 1] : y.a_cat[l - 1]);
                const int rc = input_grads_dense(h, ly, a, inp, h->A(y.a_dinp[d]), false); if (rc != SBR_OK) return rc;
            }
        }
        if (l > 0) {        // gradient wrt the level below: forward half in forward time, backwards half in reversed time
            const LayerLayout& lf = y.layer[2 * (l - 1)]; const LayerLayout& lb = y.layer[2 * (l - 1) + 1];
            SBR_LAUNCH(launch_uncat(s, h->A(y.a_dinp[0]), h->A(y.a_dinp[1]), h->blen, h->A(lf.a_dhext), h->A(lb.a_dhext), y.T, y.Bp,
                                    2 * lf.Hp, lf.Hp));
        } else if (y.E) {   // embedding table: both directions' input gradients, back in forward time, scatter-added by index
            mark(h, 5);
            SBR_LAUNCH(launch_uncat(s, h->A(y.a_dinp[0]), h->A(y.a_dinp[1]), h->blen, h->A(y.a_demb), nullptr, y.T, y.Bp, y.F * y.Ep, 0));
            { const int rc = emb_grad_scatter(h); if (rc != SBR_OK) return rc; }
        }
        if (l == 0) mark(h, 6);
    }
    if (!h->in_train_step && !h->deferred_join) return side_join(h);
    return SBR_OK;
}

extern "C" int sbr_backward_recurrent(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    if (!h->fwd_done) { sbr_set_error("sbr_backward_recurrent: call sbr_forward first"); return SBR_ESTATE; }
    h->grads_clean = false;
    return h->lay.D == 2 ? backward_bi(h) : backward_uni(h);
}

// ---------------------------------------------------------------------------------------
// the optimizer
// ---------------------------------------------------------------------------------------
// Single-call step, dense wide index-input block, the step's plain-key sort at hand (a_soff: this batch's segment offsets): the pass
// over W_in reads / clears the gradient of the touched rows only (launch_update_rows_aware).  SBR_ROW_AWARE_UPDATE=0: update_kernel.
static bool row_aware_taken(const sbr_handle* h) {
    const Layout& y = h->lay;
    return h->sw.row_aware && h->in_train_step && h->scat.wide_rows && !y.n_sparse && y.D == 1 && h->st.tail_nc < 2 &&
           h->scat.plain != SCAT_ATOMIC && !simple_gemm(h) && !simple_rec(h);
}
// [0, hi) of the parameter section on the main stream; row_aware: with the row-aware pass over layer 0's W_in
static hipError_t step_front(sbr_handle* h, size_t hi, bool row_aware) {
    if (!row_aware) return step_range(h, h->stream, 0, hi);
    const Layout& y = h->lay; const LayerLayout& l0 = y.layer[0];
    const size_t w_end = l0.p_Win + (size_t)y.cfg.input_size * y.G * l0.Hp;
    hipError_t e = step_range(h, h->stream, 0, l0.p_Win);
    if (e != hipSuccess) return e;
    if (hi < w_end) return hipErrorInvalidValue;      // (callers pass ranges that cover the block)
    e = step_rows_aware(h, h->stream);
    if (e != hipSuccess) return e;
    return step_range(h, h->stream, w_end, hi);
}

// Row-sparse blocks: dense pass over everything outside the sparse blocks, then one row-sparse step per block over the rows this
// step touched: the scatter's sorted ids / the sampled cells, or (data parallel) the ids gathered from every rank
static int update_sparse(sbr_handle* h) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    // Single rank: the index-input block's row step goes FIRST, in front of the join -- its gradient rows are this stream's own
    // work (the scatter-add), so the pass (HBM-bound, 112 us at C3) runs beside the weight-gradient GEMM the side stream is still
    // busy with instead of behind it (round 6: C3's tail behind the chain 306 -> ~265 us)
    for (int b = 0; b < y.n_sparse; ++b) {
        const SparseBlockLayout& sb = y.sparse[b];
        if (sb.kind != 0 || h->st.sp_exchanged[b] || !h->side_pending || y.D != 1 || y.E) continue;      // (plain index input, one direction: the scatter-add ran on this stream)
        // (the atomic scatter-add reads no sorted ids, so this stream has not waited for the side stream's sort yet)
        if (y.cfg.flags & SBR_FLAG_ATOMIC_SCATTER) SBR_HIP(hipStreamWaitEvent(s, h->ev_sort, 0));
        SBR_LAUNCH(step_rows(h, s, b, sparse_ids(h, b)));
        h->st.rows_stepped[b] = true;
    }
    { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
    size_t pos = 0;
    for (auto& r : sparse_float_ranges(y)) { SBR_LAUNCH(step_range(h, s, pos, r.first)); pos = r.second; }
    SBR_LAUNCH(step_range(h, s, pos, y.n_params));
    for (int b = 0; b < y.n_sparse; ++b) {
        const SparseBlockLayout& sb = y.sparse[b];
        // stepped already: beside the BPTT chain (sbr_loss_backward_output) / in front of the join above
        if ((sb.kind == 1 && h->st.wout_early) || h->st.rows_stepped[b]) continue;
        const SbrSparseIds gathered = {(const int*)h->A(sb.a_cand), nullptr, h->st.sp_ncand[b], h->st.sp_ncand[b]};
        SBR_LAUNCH(step_rows(h, s, b, h->st.sp_exchanged[b] ? gathered : sparse_ids(h, b)));
    }
    return SBR_OK;
}

// Dense updates behind a side stream that still computes dW_hid (weight-gradient GEMM + slab reduction, 240 us at C4), the last
// thing it produces.  Every other parameter is updated while it finishes: the main stream waits only for the output-layer gradients
// (recorded long ago), updates all ranges except the W_hid blocks, joins, then updates those.
static int update_around_whid(sbr_handle* h, size_t p_end, bool row_aware) {
    const Layout& y = h->lay; hipStream_t s = h->stream;
    if (y.L * y.D == 1 && y.n_params - y.layer[0].p_peep <= ((size_t)1 << 20)) {
        // small output layer (C2: 0.47 M floats): two launches instead of three; a large one (C4: 6.8 M) is better
        // updated while dW_hid finishes
        SBR_LAUNCH(step_front(h, y.layer[0].p_Whid, row_aware));          // W_in, b: main-stream gradients only
        { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
        SBR_LAUNCH(step_range(h, s, y.layer[0].p_Whid, p_end));           // W_hid, peepholes, initial states, output layer
        return SBR_OK;
    }
    SBR_HIP(hipStreamWaitEvent(s, h->ev_og, 0));
    size_t pos = 0;
    int l_from = 0;
    if (row_aware) {      // layer 0: the row-aware pass over W_in, then b
        SBR_LAUNCH(step_front(h, y.layer[0].p_Whid, row_aware));
        pos = y.layer[0].p_peep; l_from = 1;
    }
    for (int l = l_from; l < y.L * y.D; ++l) { SBR_LAUNCH(step_range(h, s, pos, y.layer[l].p_Whid)); pos = y.layer[l].p_peep; }
    SBR_LAUNCH(step_range(h, s, pos, p_end));
    { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
    for (int l = 0; l < y.L * y.D; ++l) SBR_LAUNCH(step_range(h, s, y.layer[l].p_Whid, y.layer[l].p_peep));
    return SBR_OK;
}

extern "C" int sbr_apply_update(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    const Layout& y = h->lay;
    // the step in flight is applied: it counts from whichever way this call returns (step_no until then)
    struct Count { sbr_handle* h; ~Count() { h->step_count += 1; } } count{h};
    if (h->tail_join_pending) { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
    const size_t p_end = h->st.out_early ? y.p_split : y.n_params;     // the output layer was stepped beside the BPTT chain
    const bool row_aware = row_aware_taken(h);
    h->last_row_aware = row_aware;
    if (y.n_sparse) {
        const int rc = update_sparse(h); if (rc != SBR_OK) return rc;
    } else if (h->st.tail_updated) {
        // overlapped tail of a single-call step: every stream has stepped what it produced (sbr_backward_recurrent)
    } else if (h->side_pending && h->st.tail_swapped) {
        // side stream: everything but W_hid (W_in, b from its own scatter / partials; the output layer's gradients are its
        // own too); main stream: W_hid (its own GEMM) -- no event wait in front of it; then the main stream joins the side
        // stream, normally done by then
        const LayerLayout& l0 = y.layer[0];
        SBR_LAUNCH(step_range(h, h->side, 0, p_end, l0.p_Whid, l0.p_peep - l0.p_Whid));
        SBR_LAUNCH(step_range(h, h->stream, l0.p_Whid, l0.p_peep));
        { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
    } else if (h->side_pending && h->st.og_recorded) {
        const int rc = update_around_whid(h, p_end, row_aware); if (rc != SBR_OK) return rc;
    } else {
        { const int rc = side_join(h); if (rc != SBR_OK) return rc; }
        SBR_LAUNCH(step_front(h, p_end, row_aware));
    }
    mark(h, 7);
    if (!h->in_train_step && h->timing) h->ring_used += 1;
    h->grads_clean = true;
    h->fwd_done = false;
    // the step is complete: the next batch build may trust main-stream order -- unless a road through this call ended without its join
    if (h->side_pending || h->tail_join_pending) h->bb_slow = 2;      // (another cause than step_abandoned_check's: a COMPLETED step's streams still apart)
    h->st.train_fwd_open = false;      // (the step's end, the opposite of abandoned: the reset below must not take it for one)
    step_reset(h);
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// cost and fault word; the single-call steps
// ---------------------------------------------------------------------------------------
// The recurrent kernels' bounded spin-waits raise a flag instead of hanging the GPU.  Every call that hands results to the
// host checks it (training: with the cost; inference: with the ids / scores) and CLEARS it, so that one timeout fails
// the call it belongs to and not every later call of the handle.
static int report_fault(sbr_handle* h, int fault) {
    if (!fault) return SBR_OK;
    (void)hipMemsetAsync(h->A(h->lay.a_fault), 0, sizeof(int), h->stream);
    // bit 0: cluster exchange (sbr_rec_cl.hip); bits 1, 2: publish counter / pipe gate of the pipelined kernels (sbr_rec_p.hip);
    // bit 3: a consumer of the overlapped tail (or its monitor) waited for the chain for 1.5 s; bit 4: a unit of the LDS-row
    // scatter-add was handed more ids than it has LDS rows for (launch_scatter_lds_poll sizes them: cannot happen)
    if (fault & 16)
        sbr_set_error("the LDS-row scatter-add of the overlapped tail ran out of rows (flag %d, results of this call invalid); rerun with "
                      "SBR_TAIL_SCATTER_LDS=0", fault);
    else
        sbr_set_error("a bounded wait inside the recurrent kernels gave up (flag %d, results of this call invalid); rerun with %s", fault,
                      (fault & 1) ? "SBR_CLUSTER=0" : (fault & 8) ? "SBR_TAIL_OVERLAP=0" : "SBR_X6_PIPE=0");
    return SBR_EHIP;
}
int check_fault(sbr_handle* h) {        // synchronises the stream
    int fault = 0;
    SBR_HIP(hipMemcpyAsync(&fault, h->A(h->lay.a_fault), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));
    return report_fault(h, fault);
}

extern "C" int sbr_read_cost(sbr_handle* h, float* cost_host) {
    CHECK_ARG(h && cost_host, "null argument");
    SBR_HIP(hipMemcpyAsync(cost_host, h->cost_ptr(), sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return check_fault(h);
}

extern "C" int sbr_train_step(sbr_handle* h, float* cost_host) {
    CHECK_ARG(h, "null handle");
    int rc;
    if (h->timing) h->ring_cur = h->ring_used % sbr_handle::kRing;
    h->in_train_step = true;
    struct Guard { sbr_handle* h; ~Guard() { h->in_train_step = false; } } guard{h};
    mark(h, 0);
    if ((rc = sbr_zero_grads(h)) != SBR_OK) return rc;
    if ((rc = sbr_forward(h)) != SBR_OK) return rc;
    if ((rc = sbr_loss_backward_output(h)) != SBR_OK) return rc;
    if ((rc = sbr_backward_recurrent(h)) != SBR_OK) return rc;
    // train_function returns the cost of the batch BEFORE the update (rnn_base.py:290)
    if ((rc = sbr_apply_update(h)) != SBR_OK) return rc;
    if (h->timing) h->ring_used += 1;
    if (cost_host) return sbr_read_cost(h, cost_host);
    return SBR_OK;
}

// The cost and the fault word of a lagged step reach the host through ONE one-thread kernel that stores them into pinned host memory
// and then a sequence number (round 6; before: two 4-byte device-to-host copies and an event record on the main stream between two
// steps, ~10 us of the training loop at C2).  The host reads them one step later: the number is there long before.
__global__ void lag_report_kernel(const float* cost, const int* fault, volatile float* host, int slot, unsigned seq) {
    host[slot] = *cost;
    ((volatile int*)host)[2 + slot] = *fault;
    __threadfence_system();
    ((volatile unsigned*)host)[4 + slot] = seq;
}

static int lagged_collect(sbr_handle* h, float* cost, int* have) {
    *have = 0;
    if (h->lag_pending < 0) return SBR_OK;
    const int s = h->lag_pending;
    h->lag_pending = -1;
    volatile unsigned* q = (volatile unsigned*)&h->lag_host[4 + s];
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0; *q != h->lag_seq[s]; ++spins) {
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
            SBR_HIP(hipStreamSynchronize(h->stream));      // (a step that long, or a failed one: the stream says which)
            if (*q != h->lag_seq[s]) { sbr_set_error("lagged step: its report never arrived"); return SBR_EHIP; }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *cost = h->lag_host[s];
    *have = 1;
    int fault = 0;
    memcpy(&fault, (const void*)&h->lag_host[2 + s], sizeof(int));
    return report_fault(h, fault);
}

// The report of the step just applied, for either form of the step: behind sbr_apply_update of a phase-by-phase step (a data-parallel
// driver: the cost word then holds the all-reduced, global cost) or behind sbr_train_step (sbr_train_step_lagged below).
extern "C" int sbr_cost_lagged(sbr_handle* h, float* prev_cost, int* have_prev) {
    CHECK_ARG(h && prev_cost && have_prev, "null argument");
    const int s = h->lag_slot;
    h->lag_seq[s] = ++h->lag_counter;
    lag_report_kernel<<<1, 1, 0, h->stream>>>(h->cost_ptr(), (const int*)h->A(h->lay.a_fault), h->lag_host, s, h->lag_seq[s]);
    SBR_LAUNCH(hipGetLastError());
    const int rc = lagged_collect(h, prev_cost, have_prev);          // the step before this one: normally long finished
    h->lag_pending = s;
    h->lag_slot = s ^ 1;
    return rc;
}

extern "C" int sbr_train_step_lagged(sbr_handle* h, float* prev_cost, int* have_prev) {
    CHECK_ARG(h && prev_cost && have_prev, "null argument");
    const int rc = sbr_train_step(h, nullptr);
    if (rc != SBR_OK) return rc;
    return sbr_cost_lagged(h, prev_cost, have_prev);
}

extern "C" int sbr_lagged_flush(sbr_handle* h, float* cost, int* have) {
    CHECK_ARG(h && cost && have, "null argument");
    return lagged_collect(h, cost, have);
}
