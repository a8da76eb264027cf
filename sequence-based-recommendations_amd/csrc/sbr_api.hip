// C-ABI of libsbr_rnn.so (see include/sbr_rnn.h): arena layout, Lasagne <-> device parameter
// layout conversion, batch and parameter I/O, the sparse exchange, prediction, and the debug / query / timing calls.  The
// training step itself is sbr_step.hip, the ranking and evaluation calls are sbr_rank_api.hip.
// The host side mirrors what RNNBase does around its Theano functions
// (neural_networks/rnn_base.py:175-213, :285-300, :470-515); the arithmetic lives in the kernels.
#include "sbr_common.h"
#include "sbr_state.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <stdlib.h>
#include <math.h>
#include <array>
#include <atomic>
#include <chrono>

static thread_local std::string g_err;
void sbr_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
}
extern "C" const char* sbr_last_error(void) { return g_err.c_str(); }
extern "C" int sbr_abi_version(void) { return SBR_ABI_VERSION; }


// ---------------------------------------------------------------------------------------
// Layout
// ---------------------------------------------------------------------------------------
int sbr_build_layout(const sbr_config& cfg, Layout& lay, std::string& err) {
    char buf[256];
#define LFAIL(...) do { snprintf(buf, sizeof(buf), __VA_ARGS__); err = buf; return SBR_EINVAL; } while (0)
    if (cfg.abi_version != SBR_ABI_VERSION) LFAIL("abi_version %d != %d", cfg.abi_version, SBR_ABI_VERSION);
    if (cfg.cell < 0 || cfg.cell > 2) LFAIL("Unknown layer type %d", cfg.cell);                  // recurrent_layers.py:90
    if (cfg.loss < 0 || cfg.loss > SBR_LOSS_LIN) LFAIL("Unknown loss for the RNN model (%d)", cfg.loss);     // command_parser.py:123
    if (cfg.updater < 0 || cfg.updater > 4) LFAIL("Unknown update option %d", cfg.updater);       // update_manager.py:22
    if ((cfg.flags & SBR_FLAG_BF16_PROJECTION) && (cfg.flags & SBR_FLAG_F32_MFMA))
        LFAIL("SBR_FLAG_BF16_PROJECTION and SBR_FLAG_F32_MFMA contradict each other (bf16 inputs / exact f32 products for the output projection)");
    if (cfg.n_layers < 1 || cfg.n_layers > SBR_MAX_LAYERS) LFAIL("n_layers must be in [1,%d]", SBR_MAX_LAYERS);
    for (int l = 0; l < cfg.n_layers; ++l)
        if (cfg.layers[l] < 1 || cfg.layers[l] > 1024) LFAIL("layer %d size %d out of range [1,1024]", l, cfg.layers[l]);
    if (cfg.n_items < 1 || cfg.input_size < cfg.n_items) LFAIL("need n_items >= 1 and input_size >= n_items");
    if (cfg.n_feat < 1 || cfg.n_feat > 8) LFAIL("n_feat must be in [1,8]");
    if (cfg.max_length < 1) LFAIL("max_length must be >= 1");
    if (cfg.batch_size < 1 || cfg.local_batch < 1 || cfg.local_batch > cfg.batch_size) LFAIL("need 1 <= local_batch <= batch_size");
    if (cfg.row_offset < 0 || cfg.row_offset + cfg.local_batch > cfg.batch_size) LFAIL("row_offset/local_batch outside the global batch");
    const bool margin = SBR_LOSS_IS_MARGIN(cfg.loss);
    if (cfg.loss != SBR_LOSS_CCE && !margin && cfg.n_samples < 1) LFAIL("sampled losses need n_samples >= 1");
    if (margin && (cfg.n_targets < 1 || cfg.n_targets > 4096)) LFAIL("the multi-target losses need 1 <= n_targets <= 4096");
    if (cfg.learning_rate <= 0.0f) LFAIL("learning_rate must be > 0");
    if (cfg.embedding_size < 0 || cfg.embedding_size > 4096) LFAIL("embedding_size must be in [0,4096]");
#undef LFAIL
    lay = Layout();
    lay.cfg = cfg;
    lay.L = cfg.n_layers; lay.G = sbr_gates(cfg.cell); lay.T = cfg.max_length;
    lay.B = cfg.local_batch; lay.Bp = (cfg.local_batch + 15) / 16 * 16;
    lay.N = cfg.n_items; lay.F = cfg.n_feat; lay.Bg = cfg.batch_size;
    lay.S = (cfg.loss == SBR_LOSS_CCE || margin) ? 0 : cfg.n_samples;
    lay.C = lay.Bg + lay.S;
    lay.NT = margin ? cfg.n_targets : 1;
    const int G = lay.G, T = lay.T, Bp = lay.Bp;

    lay.E = cfg.embedding_size > 0 ? cfg.embedding_size : 0;
    lay.Ep = (lay.E + 3) / 4 * 4;
    lay.D = cfg.bidirectional ? 2 : 1;
    const int D = lay.D;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += sbr_align(n); return o; };
    lay.p_Emb = lay.E ? take((size_t)cfg.input_size * lay.Ep) : 0;
    for (int l = 0; l < lay.L; ++l)
        for (int d = 0; d < D; ++d) {            // --r_bi: forward layer's parameters first (recurrent_layers.py:72-74)
            LayerLayout& y = lay.layer[l * D + d];
            y.H = cfg.layers[l]; y.Hp = sbr_pad_hidden(y.H); y.G = G;
            y.n_in = l == 0 ? (lay.E ? lay.F * lay.E : cfg.input_size) : D * cfg.layers[l - 1];
            y.n_in_p = l == 0 ? (lay.E ? lay.F * lay.Ep : cfg.input_size) : D * lay.layer[(l - 1) * D].Hp;
            y.p_Win = take((size_t)y.n_in_p * G * y.Hp);
            y.p_b = take((size_t)G * y.Hp);
            y.p_Whid = take((size_t)y.Hp * G * y.Hp);
            y.p_peep = take((size_t)3 * y.Hp);
            y.p_cinit = take(y.Hp);
            y.p_hinit = take(y.Hp);
        }
    lay.HLp = lay.layer[(lay.L - 1) * D].Hp;
    lay.HLt = D * lay.HLp;
    lay.p_split = off;
    lay.p_WoutT = take((size_t)lay.N * lay.HLt);
    lay.p_bout = take(lay.N);
    lay.n_params = off;
    lay.n_state_arrays = (cfg.updater == SBR_UPD_ADAM || cfg.updater == SBR_UPD_ADADELTA) ? 2 : 1;

    lay.s_params = 0;
    lay.s_grads = sbr_align(lay.n_params);
    lay.s_state = lay.s_grads + sbr_align(lay.n_params + 1);
    lay.s_act = lay.s_state + lay.n_state_arrays * sbr_align(lay.n_params);
    // NB: state arrays are addressed as s_state + k*n_params; n_params is already 64-aligned.

    off = 0;
    size_t maxrec = 0, max_dense_in = 0;
    for (int pl = 0; pl < lay.L * D; ++pl) {
        LayerLayout& y = lay.layer[pl];
        const int l = pl / D;
        const size_t tb = (size_t)T * Bp, tb1 = (size_t)(T + 1) * Bp;
        y.a_xt = take(tb * G * y.Hp);
        y.a_hs = take(tb1 * y.Hp);
        y.a_cs = cfg.cell == SBR_CELL_LSTM ? take(tb1 * y.Hp) : 0;
        const bool wide = y.Hp == 256 || y.Hp == 512;
        y.a_xh = wide ? take((size_t)4 * Bp * y.Hp) : 0;
        y.a_pring = wide ? take(sbr_rec_c16_ring_floats(Bp, y.Hp)) : 0;
        for (int k = 0; k < 4; ++k) y.a_g[k] = cfg.cell == SBR_CELL_VANILLA ? 0 : take(tb * y.Hp);
        y.a_dxt = take(tb * G * y.Hp);
        y.a_dhi = cfg.cell == SBR_CELL_GRU ? take(tb * y.Hp) : y.a_dxt;
        y.a_dhext = l < lay.L - 1 ? take(tb * y.Hp) : 0;
        y.a_state = take((size_t)2 * Bp * y.Hp);
        y.a_part = take((size_t)SBR_BWD_CHUNKS * Bp * (G * y.Hp + 5 * y.Hp));
        maxrec = std::max(maxrec, (size_t)y.Hp * G * y.Hp);
        if (l > 0 || lay.E) { maxrec = std::max(maxrec, (size_t)y.n_in_p * G * y.Hp); max_dense_in = std::max(max_dense_in, (size_t)y.n_in_p); }
    }
    if (lay.E) { lay.a_emb = take((size_t)T * Bp * lay.F * lay.Ep); lay.a_demb = take((size_t)T * Bp * lay.F * lay.Ep); }
    if (D == 2) {
        lay.a_Xr = take((size_t)Bp * T * lay.F);
        if (lay.E) lay.a_embr = take((size_t)T * Bp * lay.F * lay.Ep);
        for (int l = 0; l + 1 < lay.L; ++l) {
            lay.a_cat[l] = take((size_t)T * Bp * 2 * lay.layer[l * 2].Hp);
            lay.a_catr[l] = take((size_t)T * Bp * 2 * lay.layer[l * 2].Hp);
        }
        lay.a_hcat = take((size_t)Bp * lay.HLt);
        lay.a_dhl[0] = take((size_t)Bp * lay.HLp); lay.a_dhl[1] = take((size_t)Bp * lay.HLp);
        if (max_dense_in) { lay.a_dinp[0] = take((size_t)T * Bp * max_dense_in); lay.a_dinp[1] = take((size_t)T * Bp * max_dense_in); }
        if (!lay.E) {
            lay.a_s2cnt = take((size_t)cfg.input_size + 1); lay.a_s2off = take((size_t)cfg.input_size + 1);
            lay.a_s2cur = take((size_t)cfg.input_size + 1);
            lay.a_s2sid = take((size_t)T * Bp * lay.F); lay.a_s2pos = take((size_t)T * Bp * lay.F);
        }
    }
    lay.a_logits = take((size_t)Bp * ((lay.N + 3) & ~3));
    lay.a_dhlast = take((size_t)Bp * lay.HLt);
    lay.a_rowcost = take(Bp);
    if (lay.S > 0) {
        lay.a_Wc = take((size_t)lay.C * lay.HLt); lay.a_bc = take(lay.C);
        lay.a_act = take((size_t)Bp * lay.C);
        lay.a_dWc = take((size_t)lay.C * lay.HLt); lay.a_dbc = take(lay.C);
    }
    lay.a_csum = take((size_t)16 * std::max(lay.N, lay.C));
    lay.a_prof = take((size_t)3 * (Bp / 16) * 16 * 8 * 2);      // forward | backward | the one-launch head (tools/rec_prof.py, cl_prof.py, head_prof.py)
    lay.a_fault = take(64);
    lay.a_clx = take((size_t)Bp * 8 + 64);      // handshake slots: up to Bp/4 tiles x 32 members
    lay.ws_floats = std::max((size_t)1 << 20, 64 * maxrec);
    lay.a_ws = take(lay.ws_floats);
    lay.ws2_floats = 4 * lay.ws_floats;          // up to 256 weight-gradient slabs
    lay.a_ws2 = take(lay.ws2_floats);
    lay.a_X = take((size_t)Bp * T * lay.F);
    lay.a_len = take(Bp);
    lay.a_tgt = take((size_t)std::max(lay.Bg, Bp) * lay.NT);
    lay.a_dflt = margin ? take(lay.N) : 0;
    lay.a_smp = take(std::max(lay.S, 1));
    lay.a_cells = take(std::max(lay.C, 1));
    lay.a_pop = take(Bp);
    lay.a_topk = take((size_t)Bp * 64);
    lay.a_X2 = take((size_t)Bp * T * lay.F);
    lay.a_len2 = take(Bp);
    lay.a_tgt2 = take((size_t)std::max(lay.Bg, Bp) * lay.NT);
    lay.a_smp2 = take(std::max(lay.S, 1));
    lay.a_pop2 = take(Bp);
    // tail overlap (sbr_backward_recurrent): the sort's keys carry a time chunk, its counters cover chunks x ids
    lay.tail_keys = 1;
    if (lay.L == 1 && D == 1 && !lay.E && T >= 64 && T < 4096)
        lay.tail_keys = std::max(1, std::min(8, sbr_scatter_lds_ids() / std::max(1, cfg.input_size)));
    lay.a_scnt = take((size_t)lay.tail_keys * cfg.input_size + 1); lay.a_soff = take((size_t)lay.tail_keys * cfg.input_size + 1);
    lay.a_scur = take((size_t)lay.tail_keys * cfg.input_size + 1);
    lay.a_sP = take((size_t)cfg.input_size + 2);
    lay.a_sid = take((size_t)T * Bp * lay.F); lay.a_spos = take((size_t)T * Bp * lay.F);
    {   // wide index-input rows: the partial rows of the long segments' pieces (launch_scatter_wide)
        const int ghp0 = G * lay.layer[0].Hp;
        const bool wide0 = sbr_scatter_wide_rows(lay.E ? lay.Ep : 0, ghp0);
        lay.sr_slots = wide0 ? std::max(sbr_scatter_wide_slots((size_t)T * Bp * lay.F), 2 * SBR_SCAT_RANGES) : 0;
        lay.a_srpart = wide0 ? take((size_t)lay.sr_slots * ghp0) : 0;
        lay.a_srid = wide0 ? take((size_t)lay.sr_slots * 4 + 8) : 0;
    }
    lay.a_hstat = take((size_t)256 * 64 + 64);      // + the head's arrival counter and done flag
    lay.a_prog = take((size_t)Bp * 2 + 256);      // per-wave words, (a gap), the chain's clock words
    lay.a_done = take((size_t)SBR_DONE_COPIES * SBR_DONE_STRIDE);      // the monitor's word, replicated (sbr_common.h SbrPoll)
    // Row-sparse blocks (sbr_sparse.hip): the index-addressed rows of layer 0 (or of the embedding table) and, for the sampled
    // heads, the rows of W_out^T / b_out.  Taken when a step cannot touch every row anyway (more rows than candidates) or
    // when the flag forces it; SBR_FLAG_DENSE_UPDATE keeps the dense Lasagne-style pass over everything.
    lay.n_sparse = 0; lay.a_at = 0; lay.n_at = 0; lay.adam_early_exit = 0;
    // Adam's lazy replay walks a row's missed steps one by one and stops when the momentum term can no longer move the row -- at
    // most SBR_ADAM_REPLAY_CAP steps (sbr_sparse.hip).  With beta1 so close to 1 that the momentum is still alive there
    // (beta1^cap > 1e-9: beta1 > 0.9975) rows untouched for longer would lose the rest of their updates: such configurations keep
    // the dense Lasagne-style pass (exact, only slower); forcing the sparse form for them is refused.
    const bool adam_replay_unbounded = cfg.updater == SBR_UPD_ADAM && pow((double)cfg.beta1, 8190.0) > 1e-9;
    if (adam_replay_unbounded && (cfg.flags & SBR_FLAG_SPARSE_UPDATE)) {
        snprintf(buf, sizeof(buf), "row-sparse Adam steps need beta1 <= 0.9975 (beta1 = %g keeps a row's momentum alive beyond the replay cap)",
                 (double)cfg.beta1);
        err = buf; return SBR_EINVAL;
    }
    if (!(cfg.flags & SBR_FLAG_DENSE_UPDATE) && !adam_replay_unbounded) {
        const bool force = cfg.flags & SBR_FLAG_SPARSE_UPDATE;
        const int world = (lay.Bg + lay.B - 1) / lay.B;
        const long cand0 = (long)T * Bp * lay.F;
        if (force || (long)cfg.input_size > cand0) {
            SparseBlockLayout& b = lay.sparse[lay.n_sparse++];
            b = SparseBlockLayout(); b.kind = 0; b.n_rows = cfg.input_size;
            if (lay.E) { b.npairs = 1; b.off[0] = lay.p_Emb; b.width[0] = lay.Ep; b.stride[0] = lay.Ep; }
            else {
                b.npairs = D;
                for (int d = 0; d < D; ++d) { b.off[d] = lay.layer[d].p_Win; b.width[d] = G * lay.layer[d].Hp; b.stride[d] = G * lay.layer[d].Hp; }
            }
            b.max_local = (int)std::min<long>(b.n_rows, cand0);
        }
        if (lay.S > 0 && (force || lay.N > lay.C)) {
            SparseBlockLayout& b = lay.sparse[lay.n_sparse++];
            b = SparseBlockLayout(); b.kind = 1; b.n_rows = lay.N; b.npairs = 2;
            b.off[0] = lay.p_WoutT; b.width[0] = lay.HLt; b.stride[0] = lay.HLt;
            b.off[1] = lay.p_bout; b.width[1] = 1; b.stride[1] = 1;
            b.max_local = std::min(lay.N, lay.C);
        }
        for (int i = 0; i < lay.n_sparse; ++i) {
            SparseBlockLayout& b = lay.sparse[i];
            b.W = 0; for (int k = 0; k < b.npairs; ++k) b.W += b.width[k];
            b.cand_cap = world * b.max_local + 64;
            b.a_last = take(b.n_rows); b.a_mark = take(b.n_rows); b.a_cand = take(b.cand_cap); b.a_count = take(64);
        }
        if (lay.n_sparse && cfg.updater == SBR_UPD_ADAM) {
            // a_t (sbr_adam_at: what the dense launches use), tabulated until it has been == (float)lr for a while; the catch-up
            // replays missed steps with their own a_t
            const double lr = cfg.learning_rate, b1 = cfg.beta1, b2 = cfg.beta2;
            int t = 1, same = 0; double worst = 0.0, prev = 0.0;
            const int cap = 1 << 22;
            for (; t <= cap && same < 256; ++t) {
                const double a = sbr_adam_at_d(lr, b1, b2, t);
                same = ((float)a == (float)lr) ? same + 1 : 0;
                if (t > 1) worst = std::max(worst, a / prev);
                prev = a;
            }
            lay.n_at = t - 1;
            lay.adam_early_exit = (b2 > 0.0 && worst * b1 / sqrt(b2) < 0.999) ? 1 : 0;
            lay.a_at = take(lay.n_at);
        }
    }
    lay.s_end = lay.s_act + off;
    return SBR_OK;
}

void sbr_param_descs(const Layout& lay, std::vector<ParamDesc>& out) {
    out.clear();
    const int cell = lay.cfg.cell;
    static const char* lstm_g[4] = {"ingate", "forgetgate", "cell", "outgate"};       // sparse_lstm.py:240-254
    static const char* gru_g[3] = {"updategate", "resetgate", "hidden_update"};       // sparse_lstm.py:660-668
    static const char* van_g[1] = {"hidden_update"};
    const char* const* gn = cell == SBR_CELL_LSTM ? lstm_g : (cell == SBR_CELL_GRU ? gru_g : van_g);
    if (lay.E) out.push_back({"emb.W", 0, 8, 0, lay.cfg.input_size, lay.E, 2});   // lasagne EmbeddingLayer comes first
    for (int pl = 0; pl < lay.L * lay.D; ++pl) {
        const LayerLayout& y = lay.layer[pl];
        const int l = pl;      // ParamDesc.layer indexes lay.layer[] (level * D + direction)
        char pre[16];
        if (lay.D == 1) snprintf(pre, sizeof(pre), "l%d.", pl);
        else snprintf(pre, sizeof(pre), "l%d%c.", pl / 2, "fb"[pl & 1]);
        if (cell == SBR_CELL_VANILLA && (pl / lay.D > 0 || lay.E)) {
            // dense input: stock lasagne RecurrentLayer = CustomRecurrentLayer over two DenseLayers, whose get_params lists
            // its own parameter first and then the children's (recurrent_layers.py:94-104 [3P])
            out.push_back({std::string(pre) + "hid_init", l, 5, 0, 1, y.H, 2});
            out.push_back({std::string(pre) + "input_to_hidden.W", l, 0, 0, y.n_in, y.H, 2});
            out.push_back({std::string(pre) + "input_to_hidden.b", l, 2, 0, y.H, 1, 1});
            out.push_back({std::string(pre) + "hidden_to_hidden.W", l, 1, 0, y.H, y.H, 2});
            continue;
        }
        for (int g = 0; g < lay.G; ++g) {
            out.push_back({std::string(pre) + "W_in_to_" + gn[g], l, 0, g, y.n_in, y.H, 2});
            out.push_back({std::string(pre) + "W_hid_to_" + gn[g], l, 1, g, y.H, y.H, 2});
            out.push_back({std::string(pre) + "b_" + gn[g], l, 2, g, y.H, 1, 1});
        }
        if (cell == SBR_CELL_LSTM) {
            out.push_back({std::string(pre) + "W_cell_to_ingate", l, 3, 0, y.H, 1, 1});
            out.push_back({std::string(pre) + "W_cell_to_forgetgate", l, 3, 1, y.H, 1, 1});
            out.push_back({std::string(pre) + "W_cell_to_outgate", l, 3, 2, y.H, 1, 1});
            out.push_back({std::string(pre) + "cell_init", l, 4, 0, 1, y.H, 2});
        }
        out.push_back({std::string(pre) + "hid_init", l, 5, 0, 1, y.H, 2});
    }
    out.push_back({"out.W", (lay.L - 1) * lay.D, 6, 0, lay.D * lay.layer[(lay.L - 1) * lay.D].H, lay.N, 2});
    out.push_back({"out.b", (lay.L - 1) * lay.D, 7, 0, lay.N, 1, 1});
}

// position of Lasagne gate g (creation order) inside the stacked matrices:
// LSTM [i,f,c,o] = creation order (sparse_lstm.py:348-360); GRU stacks [reset, update, hidden]
// although it creates update first (sparse_lstm.py:737-749).
static inline int stacked_pos(int cell, int g) { return cell == SBR_CELL_GRU ? (g == 0 ? 1 : (g == 1 ? 0 : 2)) : g; }

// copy one Lasagne array <-> its place in a host image of a parameter-shaped section
static void convert_param(const Layout& lay, const ParamDesc& d, float* image, float* arr, bool to_image) {
    const LayerLayout& y = lay.layer[d.layer];
    const int GHp = y.G * y.Hp;
    auto mv = [&](size_t io, size_t ao) { if (to_image) image[io] = arr[ao]; else arr[ao] = image[io]; };
    const int gp = stacked_pos(lay.cfg.cell, d.gate);
    switch (d.kind) {
        case 0:
            for (int64_t r = 0; r < d.d0; ++r) {
                // stored row of logical input row r: behind an embedding f*E + e -> f*Ep + e; above another level its
                // D concatenated outputs of H units each are stored Hp apart
                int64_t rs = r;
                const int level = d.layer / lay.D;
                if (level == 0 && lay.E) rs = (r / lay.E) * lay.Ep + r % lay.E;
                else if (level > 0) { const LayerLayout& lo = lay.layer[(level - 1) * lay.D]; rs = (r / lo.H) * lo.Hp + r % lo.H; }
                for (int64_t c = 0; c < d.d1; ++c) mv(y.p_Win + rs * GHp + gp * y.Hp + c, r * d.d1 + c);
            }
            break;
        case 8: for (int64_t r = 0; r < d.d0; ++r) for (int64_t c = 0; c < d.d1; ++c) mv(lay.p_Emb + r * lay.Ep + c, r * d.d1 + c); break;
        case 1: for (int64_t r = 0; r < d.d0; ++r) for (int64_t c = 0; c < d.d1; ++c) mv(y.p_Whid + r * GHp + gp * y.Hp + c, r * d.d1 + c); break;
        case 2: for (int64_t c = 0; c < d.d0; ++c) mv(y.p_b + gp * y.Hp + c, c); break;
        case 3: for (int64_t c = 0; c < d.d0; ++c) mv(y.p_peep + d.gate * y.Hp + c, c); break;
        case 4: for (int64_t c = 0; c < d.d1; ++c) mv(y.p_cinit + c, c); break;
        case 5: for (int64_t c = 0; c < d.d1; ++c) mv(y.p_hinit + c, c); break;
        case 6:
            for (int64_t k = 0; k < d.d0; ++k) {
                const int64_t ks = (k / y.H) * lay.HLp + k % y.H;     // --r_bi: [forward H | backwards H] stored HLp apart
                for (int64_t n = 0; n < d.d1; ++n) mv(lay.p_WoutT + n * lay.HLt + ks, k * d.d1 + n);
            }
            break;
        case 7: for (int64_t n = 0; n < d.d0; ++n) mv(lay.p_bout + n, n); break;
    }
}

// ---------------------------------------------------------------------------------------
// create / destroy / parameters
// ---------------------------------------------------------------------------------------
extern "C" int sbr_arena_bytes(const sbr_config* cfg, size_t* bytes) {
    CHECK_ARG(cfg && bytes, "null argument");
    Layout lay; std::string err;
    if (sbr_build_layout(*cfg, lay, err) != SBR_OK) { sbr_set_error("%s", err.c_str()); return SBR_EINVAL; }
    *bytes = lay.s_end * sizeof(float);
    return SBR_OK;
}

// The environment, read once per engine: the only getenv calls of the library.  A test that flips a switch between two engines of
// a process gets what it asked for, and a switch flipped later does not reach an engine that is alive.
static SbrSwitches sbr_read_switches() {
    SbrSwitches sw;
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    auto flag = [&](const char* name, int dflt) { return num(name, dflt) != 0 ? 1 : 0; };
    sw.rpt = num("SBR_RPT", sw.rpt);
    sw.bwd_chunks = std::min(std::max(num("SBR_BWD_CHUNKS", sw.bwd_chunks), 1), SBR_BWD_CHUNKS);   // chunking measured neutral-to-slower at C2 (relaunch ~20 us); kept + tested
    sw.cluster = flag("SBR_CLUSTER", sw.cluster);
    sw.cl_linear = flag("SBR_CL_LINEAR", sw.cl_linear);
    sw.cl16 = flag("SBR_CL16", sw.cl16);
    sw.c16_two_level = flag("SBR_C16_TWO_LEVEL", sw.c16_two_level);
    sw.x6_pipe = num("SBR_X6_PIPE", sw.x6_pipe);
    sw.x6_f16 = flag("SBR_X6_F16", sw.x6_f16);
    sw.x6_f16_bwd = flag("SBR_X6_F16_BWD", sw.x6_f16_bwd);
    sw.fuse_gather = flag("SBR_FUSE_GATHER", sw.fuse_gather);
    sw.gemm_f16 = num("SBR_GEMM_F16", sw.gemm_f16);
    sw.wgrad_f16 = num("SBR_WGRAD_F16", sw.wgrad_f16);
    sw.tail_overlap = num("SBR_TAIL_OVERLAP", sw.tail_overlap);
    sw.tail_scatter_lds = num("SBR_TAIL_SCATTER_LDS", sw.tail_scatter_lds);
    sw.tail_trace = num("SBR_TAIL_TRACE", sw.tail_trace);
    sw.scat_range = num("SBR_SCAT_RANGE", sw.scat_range);
    sw.sparse_out_early = num("SBR_SPARSE_OUT_EARLY", sw.sparse_out_early);
    sw.head_fuse = num("SBR_HEAD_FUSE", sw.head_fuse);
    if (const char* e = getenv("SBR_HEAD_WAIT_TICKS")) sw.head_wait_ticks = strtoull(e, nullptr, 10);
    sw.out_fuse = flag("SBR_OUT_FUSE", sw.out_fuse);
    sw.row_aware = flag("SBR_ROW_AWARE_UPDATE", sw.row_aware);
    sw.cluster_rank = flag("SBR_CLUSTER_RANK", sw.cluster_rank);
    sw.cand_rank = flag("SBR_CAND_RANK", sw.cand_rank);
    return sw;
}

// the handle's priority side streams and its disable-timing events: what sbr_create makes and sbr_destroy drains and frees
static std::array<hipStream_t*, 3> handle_streams(sbr_handle* h) { return {&h->side, &h->side2, &h->side3}; }
static std::array<hipEvent_t*, 15> handle_events(sbr_handle* h) {
    return {&h->ev_fork, &h->ev_join, &h->ev_sort, &h->ev_lg, &h->ev_fill, &h->ev_og, &h->ev_tail, &h->ev_tail2, &h->ev_cells,
            &h->ev_chunk[0], &h->ev_chunk[1], &h->ev_chunk[2], &h->ev_chunk[3], &h->ev_bb, &h->ev_bbw};
}
static_assert(SBR_BWD_CHUNKS == 4, "handle_events lists ev_chunk[0 .. 3]");

extern "C" int sbr_create(const sbr_config* cfg, void* arena, size_t arena_bytes, void* stream, sbr_handle** out) {
    CHECK_ARG(cfg && out, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        sbr_set_error("no HIP device visible: libsbr_rnn.so has no CPU path");
        return SBR_EHIP;
    }
    sbr_handle* h = new sbr_handle();
    std::string err;
    if (sbr_build_layout(*cfg, h->lay, err) != SBR_OK) { sbr_set_error("%s", err.c_str()); delete h; return SBR_EINVAL; }
    const size_t need = h->lay.s_end * sizeof(float);
    h->stream = (hipStream_t)stream;
    if (arena) {
        if (arena_bytes < need || ((uintptr_t)arena & 255)) {
            sbr_set_error("arena too small (%zu < %zu bytes) or not 256-byte aligned", arena_bytes, need);
            delete h; return SBR_EINVAL;
        }
        h->arena = (float*)arena; h->own_arena = false;
    } else {
        void* p = nullptr;
        if (hipMalloc(&p, need) != hipSuccess) { sbr_set_error("hipMalloc(%zu) failed", need); delete h; return SBR_ENOMEM; }
        h->arena = (float*)p; h->own_arena = true;
    }
    sbr_param_descs(h->lay, h->descs);
    h->sw = sbr_read_switches();
    const SbrSwitches& sw = h->sw;
    // rows per workgroup of the bf16x6 recurrent kernels: the per-step latency of the chain does not depend on the
    // tile height, so take the smallest tile whose workgroups still fit the 256 CUs in one round (measured, GRU-128
    // T=200: B=512 548k seq/s at 4 rows vs 444k at 8; B=1024 856k vs 766k at 8 / 643k at 16; B=2048 1078k at 8 vs
    // 922k at 4 (two rounds) / 1047k at 16; B=4096 1380k at 16 vs 1124k at 8)
    h->rpt = sw.rpt;
    if (h->rpt != 1 && h->rpt != 2 && h->rpt != 4 && h->rpt != 8 && h->rpt != 16) { h->rpt = 4; while (h->rpt < 16 && h->lay.Bp / h->rpt > 256) h->rpt <<= 1; }
    plan_layers(h);      // every layer's recurrent kernel: the layout, the switches, the flags and rpt are all it depends on
    plan_tail(h);        // ... the overlapped tail's time chunks, and the form of layer 0's scatter-add: the same inputs
    const Layout& y = h->lay;
    h->scat = sbr_scat_plan(y.G * y.layer[0].Hp, y.E ? y.Ep : 0, y.cfg.input_size, y.T * y.Bp * y.F, y.D, (y.cfg.flags & SBR_FLAG_ATOMIC_SCATTER) != 0,
                            sw.scat_range, sw.tail_scatter_lds, h->tail_chunks, kTailScatterUnits, y.sr_slots);
    if (sw.tail_trace) {      // tools/tail_trace.py
        if (hipMalloc(&h->tail_trace, 16384 * sizeof(unsigned long long)) != hipSuccess) h->tail_trace = nullptr;
        else (void)hipMemset(h->tail_trace, 0, 16384 * sizeof(unsigned long long));
    }
    // The side stream must not share a hardware queue with the main stream (HIP multiplexes streams onto
    // GPU_MAX_HW_QUEUES = 4 queues; with RCCL's streams alive the side stream landed on the main stream's queue and
    // every "overlapped" kernel serialised: +150 us per step in the data-parallel path).  Streams of another priority
    // level get their own queues.
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    bool ok = true;
    for (hipStream_t* st : handle_streams(h)) ok = ok && hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_hi) == hipSuccess;
    for (hipEvent_t* ev : handle_events(h)) ok = ok && hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess;
#if SBR_BB_STREAM
    ok = ok && hipStreamCreateWithPriority(&h->s_bb, hipStreamNonBlocking, SBR_BB_STREAM == 2 ? prio_lo : prio_hi) == hipSuccess;
#endif
    if (!ok || hipHostMalloc((void**)&h->lag_host, 8 * sizeof(float), hipHostMallocDefault) != hipSuccess) {
        sbr_set_error("side stream creation failed"); sbr_destroy(h); return SBR_EHIP;
    }
#if !SBR_BB_STREAM
    h->s_bb = h->side3;      // (NOT a fifth stream: the device serves four hardware queues per process, a fifth stream shares one with the
                             //  main stream and the step takes 0.76 ms instead of 0.33 -- profiles/round6_variants.txt, call m)
#endif
    memset(h->lag_host, 0, 8 * sizeof(float));
    if (hipMalloc(&h->step_words, 160 * sizeof(int)) != hipSuccess || hipMemset(h->step_words, 0, 160 * sizeof(int)) != hipSuccess) {
        sbr_set_error("step boundary words: allocation failed"); sbr_destroy(h); return SBR_EHIP;
    }
    // parameters, gradients, optimizer state and batch buffers start as zeros
    // (activations too: one-off, keeps every later GEMM operand finite)
    hipError_t e = hipMemsetAsync(h->arena, 0, h->lay.s_end * sizeof(float), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { sbr_set_error("arena initialisation failed: %s", hipGetErrorString(e)); sbr_destroy(h); return SBR_EHIP; }
    if (h->lay.n_at > 0) {
        std::vector<float> at(h->lay.n_at);
        for (int t = 1; t <= h->lay.n_at; ++t) at[t - 1] = sbr_adam_at(cfg->learning_rate, cfg->beta1, cfg->beta2, t);
        e = hipMemcpy(h->A(h->lay.a_at), at.data(), at.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { sbr_set_error("a_t table upload failed: %s", hipGetErrorString(e)); sbr_destroy(h); return SBR_EHIP; }
    }
    *out = h;
    return SBR_OK;
}

extern "C" void sbr_destroy(sbr_handle* h) {
    if (!h) return;
    // work still in flight may write into what is freed below (the lagged step's report into pinned memory, a batch build into the
    // arena's second set): let every stream of the engine drain first
    (void)hipStreamSynchronize(h->stream);
    for (hipStream_t* st : handle_streams(h)) if (*st) (void)hipStreamSynchronize(*st);
    for (int r = 0; r < sbr_handle::kRing; ++r)
        for (int i = 0; i < SBR_N_PHASES; ++i) if (h->ev[r][i]) (void)hipEventDestroy(h->ev[r][i]);
    for (int r = 0; r < sbr_handle::kChain; ++r)
        for (int i = 0; i < 2; ++i) if (h->ev_ch[r][i]) (void)hipEventDestroy(h->ev_ch[r][i]);
    for (hipEvent_t* ev : handle_events(h)) if (*ev) (void)hipEventDestroy(*ev);
#if SBR_BB_STREAM
    if (h->s_bb) (void)hipStreamDestroy(h->s_bb);
#endif
    for (hipStream_t* st : handle_streams(h)) if (*st) (void)hipStreamDestroy(*st);
    if (h->lag_host) (void)hipHostFree(h->lag_host);
    if (h->own_arena && h->arena) (void)hipFree(h->arena);
    if (h->tail_trace) (void)hipFree(h->tail_trace);
    if (h->tail_slab_dev) (void)hipFree(h->tail_slab_dev);
    if (h->step_words) (void)hipFree(h->step_words);
    if (h->rank_scratch) (void)hipFree(h->rank_scratch);
    delete h;
}

extern "C" int sbr_num_params(const sbr_handle* h) { return h ? (int)h->descs.size() : SBR_EINVAL; }

extern "C" int sbr_param_shape(const sbr_handle* h, int i, int64_t dims[2], int* ndim) {
    CHECK_ARG(h && dims && ndim && i >= 0 && i < (int)h->descs.size(), "bad parameter index %d", i);
    const ParamDesc& d = h->descs[i];
    dims[0] = d.d0; dims[1] = d.ndim == 2 ? d.d1 : 1; *ndim = d.ndim;
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// row-sparse blocks (sbr_sparse.hip)
// ---------------------------------------------------------------------------------------
// every row of every sparse block current through the last applied step (before parameters are read as a whole)
int flush_lazy(sbr_handle* h, int only_kind) {
    if (!sparse_lazy(h)) return SBR_OK;
    for (int b = 0; b < h->lay.n_sparse; ++b)
        if (only_kind < 0 || h->lay.sparse[b].kind == only_kind)
            SBR_LAUNCH(launch_sparse_flush(h->stream, sparse_rows(h, b), sparse_upd(h), (int)h->step_count));
    return SBR_OK;
}
extern "C" int sbr_flush_lazy(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    return flush_lazy(h);
}

extern "C" int sbr_describe_param(const sbr_config* cfg, int i, char* name, size_t name_cap, int64_t dims[2], int* ndim) {
    CHECK_ARG(cfg && dims && ndim, "null argument");
    Layout lay; std::string err;
    if (sbr_build_layout(*cfg, lay, err) != SBR_OK) { sbr_set_error("%s", err.c_str()); return SBR_EINVAL; }
    std::vector<ParamDesc> descs;
    sbr_param_descs(lay, descs);
    CHECK_ARG(i >= 0 && i < (int)descs.size(), "parameter index %d outside [0,%d)", i, (int)descs.size());
    const ParamDesc& d = descs[i];
    if (name && name_cap) snprintf(name, name_cap, "%s", d.name.c_str());
    dims[0] = d.d0; dims[1] = d.ndim == 2 ? d.d1 : 1; *ndim = d.ndim;
    return SBR_OK;
}

extern "C" int sbr_set_params(sbr_handle* h, int n, const float* const* arrays) {
    CHECK_ARG(h && arrays && n == (int)h->descs.size(), "expected %d parameter arrays, got %d", h ? (int)h->descs.size() : -1, n);
    { const int rc = flush_lazy(h); if (rc != SBR_OK) return rc; }   // pending zero-gradient steps belong to the old values
    std::vector<float> image(h->lay.n_params, 0.0f);     // padding stays exactly zero
    for (int i = 0; i < n; ++i) {
        CHECK_ARG(arrays[i], "parameter array %d is NULL", i);
        convert_param(h->lay, h->descs[i], image.data(), const_cast<float*>(arrays[i]), true);
    }
    SBR_HIP(hipMemcpyAsync(h->P(0), image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));
    h->fwd_done = false;
    return SBR_OK;
}

static int get_section(sbr_handle* h, const float* dev, int n, float* const* arrays) {
    CHECK_ARG(h && arrays && n == (int)h->descs.size(), "expected %d parameter arrays, got %d", h ? (int)h->descs.size() : -1, n);
    std::vector<float> image(h->lay.n_params);
    SBR_HIP(hipMemcpyAsync(image.data(), dev, image.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        CHECK_ARG(arrays[i], "parameter array %d is NULL", i);
        convert_param(h->lay, h->descs[i], image.data(), arrays[i], false);
    }
    return SBR_OK;
}
extern "C" int sbr_get_params(sbr_handle* h, int n, float* const* arrays) {
    CHECK_ARG(h, "null handle");
    { const int rc = flush_lazy(h); if (rc != SBR_OK) return rc; }
    return get_section(h, h->P(0), n, arrays);
}
extern "C" int sbr_get_grads(sbr_handle* h, int n, float* const* arrays) { return get_section(h, h ? h->Gd(0) : nullptr, n, arrays); }

extern "C" int sbr_section(sbr_handle* h, int which, void** dev_ptr, size_t* n_floats, size_t* split_floats) {
    CHECK_ARG(h && dev_ptr && n_floats, "null argument");
    const Layout& y = h->lay;
    if (split_floats) *split_floats = y.p_split;
    if (which == 0 || which == 2) { const int rc = flush_lazy(h); if (rc != SBR_OK) return rc; }   // current at the time of the call
    switch (which) {
        case 0: *dev_ptr = h->P(0); *n_floats = y.n_params; return SBR_OK;
        case 1: *dev_ptr = h->Gd(0); *n_floats = y.n_params + 1; return SBR_OK;
        case 2: *dev_ptr = h->St(0, 0); *n_floats = y.n_state_arrays * y.n_params; return SBR_OK;
    }
    sbr_set_error("unknown section %d", which);
    return SBR_EINVAL;
}

// ---------------------------------------------------------------------------------------
// the whole training state as one host blob (include/sbr_rnn.h "Training state"; head and its checks: sbr_state.h)
// ---------------------------------------------------------------------------------------
// What fixes the blob's layout.  Nothing of local_batch / row_offset: data-parallel replicas hold the same state.
struct EngineStateFp {
    uint64_t n_params, p_split;
    uint32_t n_state, updater, n_sparse, pad;
    uint32_t kind[2], rows[2], width[2];
    uint64_t shapes;        // FNV-1a over the logical shapes of the parameter list: widths that pad alike (20 and 30 units) are still two models
};
static EngineStateFp engine_state_fp(const sbr_handle* h) {
    const Layout& y = h->lay;
    EngineStateFp f;
    memset(&f, 0, sizeof(f));
    f.shapes = 0xcbf29ce484222325ull;
    for (const ParamDesc& d : h->descs)
        for (int64_t v : {(int64_t)d.ndim, d.d0, d.ndim == 2 ? d.d1 : (int64_t)1})
            for (int i = 0; i < 8; ++i) { f.shapes ^= (uint64_t)(v >> (8 * i)) & 0xff; f.shapes *= 0x100000001b3ull; }
    f.n_params = y.n_params; f.p_split = y.p_split;
    f.n_state = (uint32_t)y.n_state_arrays; f.updater = (uint32_t)y.cfg.updater; f.n_sparse = (uint32_t)y.n_sparse;
    for (int b = 0; b < y.n_sparse; ++b) { f.kind[b] = (uint32_t)y.sparse[b].kind; f.rows[b] = (uint32_t)y.sparse[b].n_rows; f.width[b] = (uint32_t)y.sparse[b].W; }
    return f;
}
// head | fingerprint | step_count | parameter section (padded, as it lies in the arena) | state arrays | a_last of every sparse block
static const size_t kEngineStateFixed = sizeof(SbrStateHead) + sizeof(EngineStateFp) + sizeof(int64_t);
static size_t engine_state_bytes(const Layout& y) {
    size_t n = kEngineStateFixed + (1 + y.n_state_arrays) * y.n_params * sizeof(float);
    for (int b = 0; b < y.n_sparse; ++b) n += (size_t)y.sparse[b].n_rows * sizeof(int);
    return n;
}
static int engine_sync_all(sbr_handle* h) {
    SBR_HIP(hipStreamSynchronize(h->stream));
    for (hipStream_t* st : handle_streams(h)) if (*st) SBR_HIP(hipStreamSynchronize(*st));
    return SBR_OK;
}

extern "C" int sbr_state_bytes(sbr_handle* h, size_t* bytes) {
    CHECK_ARG(h && bytes, "null argument");
    *bytes = engine_state_bytes(h->lay);
    return SBR_OK;
}

extern "C" int sbr_state_save(sbr_handle* h, void* blob, size_t cap, size_t* written) {
    CHECK_ARG(h && blob && written, "null argument");
    const Layout& y = h->lay;
    if (h->st.step_open || h->st.train_fwd_open) { sbr_set_error("sbr_state_save: a training step is open (finish it with sbr_apply_update)"); return SBR_ESTATE; }
    if (h->lag_pending >= 0) { sbr_set_error("sbr_state_save: a lagged cost is pending (collect it with sbr_lagged_flush)"); return SBR_ESTATE; }
    const size_t need = engine_state_bytes(y);
    CHECK_ARG(cap >= need, "sbr_state_save: the state takes %zu bytes, the buffer holds %zu", need, cap);
    // no launch, no flush: the lazily stepped rows and their `last` words are saved as they stand
    { const int rc = engine_sync_all(h); if (rc != SBR_OK) return rc; }
    char* p = (char*)blob;
    const SbrStateHead hd = sbr_state_head(SBR_STATE_ENGINE, need);
    const EngineStateFp fp = engine_state_fp(h);
    const int64_t steps = h->step_count;
    memcpy(p, &hd, sizeof(hd)); p += sizeof(hd);
    memcpy(p, &fp, sizeof(fp)); p += sizeof(fp);
    memcpy(p, &steps, sizeof(steps)); p += sizeof(steps);
    const size_t sec = y.n_params * sizeof(float);
    SBR_HIP(hipMemcpyAsync(p, h->P(0), sec, hipMemcpyDeviceToHost, h->stream)); p += sec;
    for (size_t k = 0; k < y.n_state_arrays; ++k) { SBR_HIP(hipMemcpyAsync(p, h->St((int)k, 0), sec, hipMemcpyDeviceToHost, h->stream)); p += sec; }
    for (int b = 0; b < y.n_sparse; ++b) {
        const size_t n = (size_t)y.sparse[b].n_rows * sizeof(int);
        SBR_HIP(hipMemcpyAsync(p, h->A(y.sparse[b].a_last), n, hipMemcpyDeviceToHost, h->stream)); p += n;
    }
    SBR_HIP(hipStreamSynchronize(h->stream));
    *written = need;
    return SBR_OK;
}

extern "C" int sbr_state_load(sbr_handle* h, const void* blob, size_t bytes) {
    CHECK_ARG(h, "null handle");
    const Layout& y = h->lay;
    if (h->st.step_open || h->st.train_fwd_open) { sbr_set_error("sbr_state_load: a training step is open (finish it with sbr_apply_update)"); return SBR_ESTATE; }
    // everything is checked before anything is written
    { const int rc = sbr_state_check_head(blob, bytes, SBR_STATE_ENGINE, "sbr_state_load"); if (rc != SBR_OK) return rc; }
    CHECK_ARG(bytes >= kEngineStateFixed, "sbr_state_load: a blob of %zu bytes is shorter than its fixed part (%zu)", bytes, kEngineStateFixed);
    const char* p = (const char*)blob + sizeof(SbrStateHead);
    EngineStateFp got; const EngineStateFp fp = engine_state_fp(h);
    int64_t steps = 0;
    memcpy(&got, p, sizeof(got)); p += sizeof(got);
    memcpy(&steps, p, sizeof(steps)); p += sizeof(steps);
    CHECK_ARG(got.n_params == fp.n_params && got.p_split == fp.p_split,
              "sbr_state_load: the blob holds %llu parameters (output layer at %llu), this engine %llu (at %llu): another architecture",
              (unsigned long long)got.n_params, (unsigned long long)got.p_split, (unsigned long long)fp.n_params, (unsigned long long)fp.p_split);
    CHECK_ARG(got.shapes == fp.shapes, "sbr_state_load: the blob's parameter arrays have other shapes than this engine's (other layer widths behind the same padding)");
    CHECK_ARG(got.updater == fp.updater && got.n_state == fp.n_state, "sbr_state_load: the blob is of updater %u with %u state arrays, this engine of updater %u with %u",
              got.updater, got.n_state, fp.updater, fp.n_state);
    CHECK_ARG(got.n_sparse == fp.n_sparse, "sbr_state_load: the blob has %u row-sparse blocks, this engine %u", got.n_sparse, fp.n_sparse);
    for (int b = 0; b < y.n_sparse; ++b)
        CHECK_ARG(got.kind[b] == fp.kind[b] && got.rows[b] == fp.rows[b] && got.width[b] == fp.width[b],
                  "sbr_state_load: row-sparse block %d is kind %u, %u rows of %u floats in the blob; kind %u, %u rows of %u here", b, got.kind[b],
                  got.rows[b], got.width[b], fp.kind[b], fp.rows[b], fp.width[b]);
    CHECK_ARG(bytes == engine_state_bytes(y), "sbr_state_load: the state of this engine takes %zu bytes, the blob has %zu", engine_state_bytes(y), bytes);
    CHECK_ARG(steps >= 0, "sbr_state_load: step count %lld", (long long)steps);
    const size_t sec = y.n_params * sizeof(float);
    {   // a row is current through a step that has been applied
        const char* q = p + (1 + y.n_state_arrays) * sec;
        for (int b = 0; b < y.n_sparse; ++b)
            for (int r = 0; r < y.sparse[b].n_rows; ++r, q += sizeof(int)) {
                int last; memcpy(&last, q, sizeof(int));
                CHECK_ARG(last >= 0 && last <= steps, "sbr_state_load: row %d of block %d is current through step %d of %lld", r, b, last, (long long)steps);
            }
    }
    // from here on the engine changes.  Work in flight may still read what is overwritten: let every stream drain first
    { const int rc = engine_sync_all(h); if (rc != SBR_OK) return rc; }
    SBR_HIP(hipMemcpyAsync(h->P(0), p, sec, hipMemcpyHostToDevice, h->stream)); p += sec;
    for (size_t k = 0; k < y.n_state_arrays; ++k) { SBR_HIP(hipMemcpyAsync(h->St((int)k, 0), p, sec, hipMemcpyHostToDevice, h->stream)); p += sec; }
    for (int b = 0; b < y.n_sparse; ++b) {
        const size_t n = (size_t)y.sparse[b].n_rows * sizeof(int);
        SBR_HIP(hipMemcpyAsync(h->A(y.sparse[b].a_last), p, n, hipMemcpyHostToDevice, h->stream)); p += n;
    }
    // a fresh step boundary: no gradients, no batch, no forward, no open step, no report under way
    SBR_HIP(hipMemsetAsync(h->Gd(0), 0, (y.n_params + 1) * sizeof(float), h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));      // the caller's blob may be freed on return
    h->step_count = steps;
    h->grads_clean = true;
    h->fwd_done = false; h->have_batch = false; h->bb_unread = false;
    step_reset(h);
    h->lag_pending = -1;
    if (h->bb_slow < 1) h->bb_slow = 1;             // the next build trusts no record made before the load
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// batch
// ---------------------------------------------------------------------------------------
extern "C" int sbr_set_default_target(sbr_handle* h, const float* default_target) {
    CHECK_ARG(h, "null handle");
    const Layout& y = h->lay;
    CHECK_ARG(SBR_LOSS_IS_MARGIN(y.cfg.loss), "only the multi-target losses (hinge / logit / logsig) have a default target");
    if (default_target) SBR_HIP(hipMemcpyAsync(h->A(y.a_dflt), default_target, (size_t)y.N * sizeof(float), hipMemcpyHostToDevice, h->stream));
    else SBR_HIP(hipMemsetAsync(h->A(y.a_dflt), 0, (size_t)y.N * sizeof(float), h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));
    return SBR_OK;
}

extern "C" int sbr_set_batch(sbr_handle* h, const int32_t* X, const int32_t* lengths, const int32_t* target,
                             const int32_t* samples, const float* pop, int n_rows, int on_device) {
    CHECK_ARG(h && X && lengths, "null X / lengths");
    const Layout& y = h->lay;
    CHECK_ARG(n_rows >= 1 && n_rows <= y.B, "n_rows %d outside [1,%d]", n_rows, y.B);
    const bool margin = SBR_LOSS_IS_MARGIN(y.cfg.loss);
    const int n_tgt = y.S > 0 ? y.Bg : n_rows * y.NT;
    if (!on_device) {   // the reference would raise IndexError inside Theano for bad ids; check on host
        for (size_t i = 0; i < (size_t)n_rows * y.T * y.F; ++i)
            CHECK_ARG(X[i] >= 0 && X[i] < y.cfg.input_size, "input index %d out of range [0,%d)", X[i], y.cfg.input_size);
        for (int i = 0; i < n_rows; ++i) CHECK_ARG(lengths[i] >= 0 && lengths[i] <= y.T, "length %d outside [0,%d]", lengths[i], y.T);
        if (target) for (int i = 0; i < n_tgt; ++i) CHECK_ARG((target[i] >= 0 || (margin && target[i] == -1)) && target[i] < y.N, "target %d out of range", target[i]);
        if (samples) for (int i = 0; i < y.S; ++i) CHECK_ARG(samples[i] >= 0 && samples[i] < y.N, "sample %d out of range", samples[i]);
    }
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t s = h->stream;
    h->bX = (const int*)h->A(y.a_X); h->blen = (const int*)h->A(y.a_len); h->btgt = (const int*)h->A(y.a_tgt);
    h->bsmp = (const int*)h->A(y.a_smp); h->bpop = h->A(y.a_pop);
    h->bb_set = 0; h->bb_unread = false;      // (written on the main stream, behind every reader of the set: sbr_build_batch's stream was joined when it built)
    if (on_device && n_rows == y.Bp && (pop || margin)) {
        // device-resident inputs that cover every (padded) row: use them in place, no copies.  The caller
        // keeps them alive and unchanged until the step has run (stream order), as with any device input.
        h->bX = X; h->blen = lengths; if (pop) h->bpop = pop;
        if (target) h->btgt = target;
        if (samples && y.S > 0) h->bsmp = samples;
    } else {
        if (n_rows < y.Bp) {   // padded rows: index 0, length 0, popularity 1
            if (margin) SBR_HIP(hipMemsetAsync(h->A(y.a_tgt), 0xFF, (size_t)y.Bp * y.NT * sizeof(int), s));   // no positives
            SBR_HIP(hipMemsetAsync(h->A(y.a_X), 0, (size_t)y.Bp * y.T * y.F * sizeof(int), s));
            SBR_HIP(hipMemsetAsync(h->A(y.a_len), 0, (size_t)y.Bp * sizeof(int), s));
            SBR_LAUNCH(launch_fill(s, h->A(y.a_pop), 1.0f, y.Bp));
        }
        SBR_HIP(hipMemcpyAsync(h->A(y.a_X), X, (size_t)n_rows * y.T * y.F * sizeof(int), kind, s));
        SBR_HIP(hipMemcpyAsync(h->A(y.a_len), lengths, (size_t)n_rows * sizeof(int), kind, s));
        if (target) SBR_HIP(hipMemcpyAsync(h->A(y.a_tgt), target, (size_t)n_tgt * sizeof(int), kind, s));
        if (samples && y.S > 0) SBR_HIP(hipMemcpyAsync(h->A(y.a_smp), samples, (size_t)y.S * sizeof(int), kind, s));
        if (pop) SBR_HIP(hipMemcpyAsync(h->A(y.a_pop), pop, (size_t)n_rows * sizeof(float), kind, s));
        else SBR_LAUNCH(launch_fill(s, h->A(y.a_pop), 1.0f, y.Bp));
    }
    if (!on_device) SBR_HIP(hipStreamSynchronize(s));   // caller's host arrays may be freed on return
    h->n_rows = n_rows; h->have_batch = true; h->fwd_done = false;
    return SBR_OK;
}

extern "C" int sbr_zero_grads(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    step_reset(h);                                // nothing of the step before, however it ended, reaches this one
    h->st.step_open = true;                       // a training step begins: sbr_forward may start its batch-only work
    if (!h->in_train_step && h->timing) {         // phase-by-phase step (data-parallel driver): this call opens the step
        h->ring_cur = h->ring_used % sbr_handle::kRing;
        mark(h, 0);
    }
    if (h->grads_clean) return SBR_OK;            // the optimizer kernel zeroes every gradient it consumes
    SBR_HIP(hipMemsetAsync(h->Gd(0), 0, (h->lay.n_params + 1) * sizeof(float), h->stream));
    h->grads_clean = true;
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// data-parallel exchange of the row-sparse blocks (include/sbr_rnn.h)
// ---------------------------------------------------------------------------------------
extern "C" int sbr_sparse_info(sbr_handle* h, int b, int64_t* n_rows, int64_t* row_floats, int64_t* max_local_rows) {
    CHECK_ARG(h, "null handle");
    CHECK_ARG(b >= 0 && b < h->lay.n_sparse, "sparse block %d outside [0,%d)", b, h->lay.n_sparse);
    const SparseBlockLayout& sb = h->lay.sparse[b];
    if (n_rows) *n_rows = sb.n_rows;
    if (row_floats) *row_floats = sb.W;
    if (max_local_rows) *max_local_rows = sb.max_local;
    return SBR_OK;
}

// this rank's touched rows of block b, deduplicated, into ids_out / rows_out; their running count into *count (NULL: the block's a_count)
static int sparse_pack_into(sbr_handle* h, int b, int* ids_out, float* rows_out, int* count) {
    CHECK_ARG(b >= 0 && b < h->lay.n_sparse, "sparse block %d outside [0,%d)", b, h->lay.n_sparse);
    const SparseBlockLayout& sb = h->lay.sparse[b];
    if (!count) count = (int*)h->A(sb.a_count);
    { const int rc = side_join(h); if (rc != SBR_OK) return rc; }      // the block's gradients come from both streams
    const int epoch = ++h->sp_epoch;
    const SbrSparseIds c = sparse_ids(h, b);
    SBR_LAUNCH(launch_sparse_pack(h->stream, sparse_rows(h, b), c.list, c.n_dev, c.n_host, c.n_max, (int*)h->A(sb.a_mark), epoch, ids_out, rows_out,
                                  sb.W, count));
    h->st.sp_exchanged[b] = 1; h->st.sp_ncand[b] = 0;      // (a second pack of one step starts its candidate list again)
    return SBR_OK;
}

extern "C" int sbr_sparse_pack(sbr_handle* h, int b, int32_t* ids_dev, float* rows_dev, int32_t* count_host) {
    CHECK_ARG(h && ids_dev && rows_dev && count_host, "null argument");
    { const int rc = sparse_pack_into(h, b, ids_dev, rows_dev, nullptr); if (rc != SBR_OK) return rc; }
    SBR_HIP(hipMemcpyAsync(count_host, h->A(h->lay.sparse[b].a_count), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));
    return SBR_OK;
}

extern "C" int sbr_sparse_unpack_add(sbr_handle* h, int b, const int32_t* ids_dev, const float* rows_dev, int count) {
    CHECK_ARG(h && (count == 0 || (ids_dev && rows_dev)), "null argument");
    CHECK_ARG(b >= 0 && b < h->lay.n_sparse, "sparse block %d outside [0,%d)", b, h->lay.n_sparse);
    const SparseBlockLayout& sb = h->lay.sparse[b];
    if (!h->st.sp_exchanged[b]) { sbr_set_error("sbr_sparse_unpack_add: call sbr_sparse_pack for this step first"); return SBR_ESTATE; }
    CHECK_ARG(count >= 0 && h->st.sp_ncand[b] + count <= sb.cand_cap, "%d + %d rows exceed the candidate capacity %d", h->st.sp_ncand[b], count, sb.cand_cap);
    SBR_LAUNCH(launch_sparse_unpack_add(h->stream, sparse_rows(h, b), ids_dev, rows_dev, count, sb.W, (int*)h->A(sb.a_cand) + h->st.sp_ncand[b]));
    h->st.sp_ncand[b] += count;
    h->grads_clean = false;
    return SBR_OK;
}

extern "C" int sbr_sparse_pack_device(sbr_handle* h, int b, int32_t* ids_dev, float* rows_dev) {
    CHECK_ARG(h && ids_dev && rows_dev, "null argument");
    return sparse_pack_into(h, b, ids_dev + 1, rows_dev, ids_dev);      // the running count of the pack kernel IS the in-band word ids_dev[0]
}

extern "C" int sbr_sparse_unpack_add_all(sbr_handle* h, int b, const int32_t* ids_all, const float* rows_all, int world) {
    CHECK_ARG(h && ids_all && rows_all, "null argument");
    CHECK_ARG(b >= 0 && b < h->lay.n_sparse, "sparse block %d outside [0,%d)", b, h->lay.n_sparse);
    const SparseBlockLayout& sb = h->lay.sparse[b];
    if (!h->st.sp_exchanged[b]) { sbr_set_error("sbr_sparse_unpack_add_all: call sbr_sparse_pack_device for this step first"); return SBR_ESTATE; }
    const int cap = sb.max_local;
    CHECK_ARG(world >= 1 && h->st.sp_ncand[b] == 0 && (long)world * cap <= sb.cand_cap, "%d ranks x %d rows exceed the candidate capacity %d", world, cap, sb.cand_cap);
    for (int r = 0; r < world; ++r)      // rank order, one stream: every replica adds in the same order
        SBR_LAUNCH(launch_sparse_unpack_add_dev(h->stream, sparse_rows(h, b), ids_all + (size_t)r * (cap + 1), rows_all + (size_t)r * cap * sb.W,
                                                cap, sb.W, (int*)h->A(sb.a_cand) + (size_t)r * cap));
    h->st.sp_ncand[b] = world * cap;          // slots beyond a rank's count hold -1 (skipped by the row-sparse step)
    h->grads_clean = false;
    return SBR_OK;
}

std::vector<std::pair<size_t, size_t>> sparse_float_ranges(const Layout& y) {
    std::vector<std::pair<size_t, size_t>> skip;
    for (int b = 0; b < y.n_sparse; ++b)
        for (int k = 0; k < y.sparse[b].npairs; ++k)
            skip.push_back({y.sparse[b].off[k], y.sparse[b].off[k] + (size_t)y.sparse[b].n_rows * y.sparse[b].stride[k]});
    std::sort(skip.begin(), skip.end());
    return skip;
}

extern "C" int sbr_dense_ranges(sbr_handle* h, int cap, int64_t* lo, int64_t* hi, int* n) {
    CHECK_ARG(h && lo && hi && n, "null argument");
    const Layout& y = h->lay;
    const std::vector<std::pair<size_t, size_t>> skip = sparse_float_ranges(y);
    std::vector<std::pair<size_t, size_t>> out;
    size_t pos = 0;
    // ranges never straddle the output-layer split: the part in front of it is complete later than the part behind it
    auto emit = [&](size_t a, size_t b) {
        if (b <= a) return;
        if (a < y.p_split && b > y.p_split) { out.push_back({a, y.p_split}); out.push_back({y.p_split, b}); }
        else out.push_back({a, b});
    };
    for (const auto& r : skip) { emit(pos, r.first); pos = r.second; }
    emit(pos, y.n_params + 1);                        // the batch cost rides behind the last parameter
    CHECK_ARG((int)out.size() <= cap, "%d ranges, capacity %d", (int)out.size(), cap);
    for (size_t i = 0; i < out.size(); ++i) { lo[i] = (int64_t)out[i].first; hi[i] = (int64_t)out[i].second; }
    *n = (int)out.size();
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// predict (the ranking calls, sbr_topk among them: sbr_rank_api.hip)
// ---------------------------------------------------------------------------------------
// The projection of `n_rows` rows of states `rows_in` [n_rows][HLt] into scores `out` [n_rows][N]: the GEMM in scores_gemm_mode, then
// the bias pass.  ONE statement of the launch pair, so that whatever state is projected -- h_last into a_logits (full_scores), one or
// several slots of the top layer's a_hs (sbr_evaluate_positions) -- gives the floats sbr_rank ranks for a row in that state: in
// scores_gemm_mode (exact f32 without a workspace, hence without split-K; or the one-pass bf16 kernel) an output element is one
// accumulation chain over K whose order does not depend on the rows a launch carries (projection_mode, sbr_step.hip).
int project_rows(sbr_handle* h, const float* rows_in, int n_rows, float* out, int do_softmax) {
    const Layout& y = h->lay;
    SBR_LAUNCH(launch_gemm(h->stream, scores_gemm_mode(h), gemm_rowmajor(rows_in, y.HLt), gemm_transposed(h->P(y.p_WoutT), y.HLt), out, y.N,
                           n_rows, y.N, y.HLt));
    SBR_LAUNCH(launch_softmax_rows(h->stream, out, h->P(y.p_bout), n_rows, y.N, do_softmax));
    return SBR_OK;
}

int full_scores(sbr_handle* h, int do_softmax) {
    int rc;
    if ((rc = forward_current(h)) != SBR_OK) return rc;    // every item is scored: all of W_out^T / b_out must be current
    return project_rows(h, h_last(h), h->n_rows, h->A(h->lay.a_logits), do_softmax);
}

extern "C" int sbr_predict_scores(sbr_handle* h, int probs, float* out_host) {
    CHECK_ARG(h, "null handle");
    if (!h->have_batch) { sbr_set_error("sbr_predict_scores: no batch set"); return SBR_ESTATE; }
    const Layout& y = h->lay;
    const int rc = full_scores(h, (probs || y.cfg.loss == SBR_LOSS_CCE) ? 1 : 0);
    if (rc != SBR_OK) return rc;
    if (out_host) {
        SBR_HIP(hipMemcpyAsync(out_host, h->A(y.a_logits), (size_t)h->n_rows * y.N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        return check_fault(h);      // a forward that gave up must not hand out scores
    }
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------
// debug / timing
// ---------------------------------------------------------------------------------------
extern "C" int sbr_debug_buffer(sbr_handle* h, const char* name, void** dev_ptr, size_t* n_floats) {
    CHECK_ARG(h && name && dev_ptr && n_floats, "null argument");
    const Layout& y = h->lay;
    const std::string nm(name);
    const size_t tb = (size_t)y.T * y.Bp;
    if (nm == "h_last") { *dev_ptr = h_last(h); *n_floats = (size_t)y.Bp * y.HLt; return SBR_OK; }
    if (nm == "logits") { *dev_ptr = h->A(y.a_logits); *n_floats = (size_t)y.Bp * ((y.N + 3) & ~3); return SBR_OK; }
    if (nm == "dh_last") { *dev_ptr = h->A(y.a_dhlast); *n_floats = (size_t)y.Bp * y.HLt; return SBR_OK; }
    if (nm == "batch_X") { *dev_ptr = (void*)h->bX; *n_floats = (size_t)y.Bp * y.T * y.F; return SBR_OK; }
    if (nm == "batch_lengths") { *dev_ptr = (void*)h->blen; *n_floats = y.Bp; return SBR_OK; }
    if (nm == "batch_target") { *dev_ptr = (void*)h->btgt; *n_floats = y.S > 0 ? y.Bg : (size_t)y.Bp * y.NT; return SBR_OK; }
    if (nm == "batch_pop") { *dev_ptr = (void*)h->bpop; *n_floats = y.Bp; return SBR_OK; }
    if (nm == "batch_samples") { *dev_ptr = (void*)h->bsmp; *n_floats = y.S; return SBR_OK; }
    if (nm == "prof") { *dev_ptr = h->A(y.a_prof); *n_floats = (size_t)2 * (y.Bp / 16) * 16 * 8 * 2; return SBR_OK; }
    if (nm == "prof_head") { *dev_ptr = h->A(y.a_prof) + (size_t)2 * (y.Bp / 16) * 16 * 8 * 2; *n_floats = (size_t)(y.Bp / 16) * 16 * 8 * 2; return SBR_OK; }
    if (nm == "tail_trace" && h->tail_trace) { *dev_ptr = h->tail_trace; *n_floats = 2 * 16384; return SBR_OK; }
    if (nm == "tail_chain_clock") { *dev_ptr = (int*)h->A(y.a_prog) + (y.Bp / h->rpt) * 8 + 128; *n_floats = 8; return SBR_OK; }
    if (nm == "rowcost") { *dev_ptr = h->A(y.a_rowcost); *n_floats = y.Bp; return SBR_OK; }
    if (nm == "act" && y.S > 0) { *dev_ptr = h->A(y.a_act); *n_floats = (size_t)y.Bp * y.C; return SBR_OK; }
    for (int l = 0; l < y.L; ++l) {
        const LayerLayout& ly = y.layer[l];
        const std::string sfx = std::to_string(l);
        if (nm == "xt" + sfx) { *dev_ptr = h->A(ly.a_xt); *n_floats = tb * y.G * ly.Hp; return SBR_OK; }
        if (nm == "hs" + sfx) { *dev_ptr = h->A(ly.a_hs); *n_floats = (tb + y.Bp) * ly.Hp; return SBR_OK; }
        if (nm == "cs" + sfx && y.cfg.cell == SBR_CELL_LSTM) { *dev_ptr = h->A(ly.a_cs); *n_floats = (tb + y.Bp) * ly.Hp; return SBR_OK; }
        if (nm == "dxt" + sfx) { *dev_ptr = h->A(ly.a_dxt); *n_floats = tb * y.G * ly.Hp; return SBR_OK; }
        if (nm == "dhi" + sfx) { *dev_ptr = h->A(ly.a_dhi); *n_floats = tb * (y.cfg.cell == SBR_CELL_GRU ? 1 : y.G) * ly.Hp; return SBR_OK; }
    }
    sbr_set_error("unknown debug buffer '%s'", name);
    return SBR_EINVAL;
}

extern "C" int sbr_copy_to_host(sbr_handle* h, const void* dev_ptr, float* host, size_t n_floats) {
    CHECK_ARG(h && dev_ptr && host, "null argument");
    SBR_HIP(hipMemcpyAsync(host, dev_ptr, n_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));
    return SBR_OK;
}

extern "C" int sbr_synchronize(sbr_handle* h) {
    CHECK_ARG(h, "null handle");
    SBR_HIP(hipStreamSynchronize(h->stream));
    return SBR_OK;
}

extern "C" int sbr_debug_gemm(void* stream, const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                              float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, float* ws,
                              size_t ws_floats, int32_t exact_f32) {
    CHECK_ARG(A && B && C, "null operand");
    static const GemmMode modes[6] = {
        // simple, exact_f32, planes, sa, sb, no_wide, one_pass
        {false, false, 0, 1.0f, 1.0f, false, false},      // 0: bf16x6 where the shape allows it
        {false, true, 0, 1.0f, 1.0f, false, false},       // 1: the exact-f32 kernel
        {false, false, 0, 1.0f, 1.0f, false, true},       // 2: plain bf16 in one pass (SBR_FLAG_BF16_PROJECTION)
        {false, false, 2, 1.0f, 1.0f, false, false},      // 3: the two-plane fp16 split (three MFMAs): what the step's logits GEMM takes
        {false, false, 2, 1.0f, 1.0f, true, false},       // 4: as 3, kept on the 128-wide tile
        {false, false, 0, 1.0f, 1.0f, true, true},        // 5: as 2, kept on the 128-wide tile
    };
    SBR_LAUNCH(launch_gemm((hipStream_t)stream, modes[exact_f32 >= 0 && exact_f32 <= 5 ? exact_f32 : 0], GemmOperand{A, (long)sam, (long)sak, 0}, GemmOperand{B, (long)sbk, (long)sbn, 0},
                           C, (long)ldc, M, N, K, bias, ws, ws_floats));
    return SBR_OK;
}

// a foreign kernel that holds CUs for a while (include/sbr_rnn.h: test hook)
__global__ void __launch_bounds__(256) occupy_kernel(unsigned long long ticks, int* sink) {
    extern __shared__ int occ_lds[];
    occ_lds[threadIdx.x] = (int)threadIdx.x;
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
    if (occ_lds[(threadIdx.x + 1) & 255] == -7) *sink = 1;      // (keeps the LDS claim alive)
}
extern "C" int sbr_debug_occupy(sbr_handle* h, int workgroups, int lds_kb, int milliseconds) {
    CHECK_ARG(h && workgroups >= 0 && workgroups <= 4096 && lds_kb >= 0 && lds_kb <= 160 && milliseconds >= 0 && milliseconds <= 10000, "bad argument");
    static hipStream_t occ = nullptr;
    if (!occ) SBR_HIP(hipStreamCreateWithFlags(&occ, hipStreamNonBlocking));
    if (workgroups == 0) { SBR_HIP(hipStreamSynchronize(occ)); return SBR_OK; }
    const size_t lds = std::max<size_t>(1024, (size_t)lds_kb * 1024);
    SBR_DYN_LDS(occupy_kernel, lds);
    occupy_kernel<<<workgroups, 256, lds, occ>>>((unsigned long long)milliseconds * 100000ull, (int*)h->A(h->lay.a_fault) + 1);
    SBR_LAUNCH(hipGetLastError());
    return SBR_OK;
}

extern "C" int sbr_query(sbr_handle* h, const char* what, int64_t* value) {
    CHECK_ARG(h && what && value, "null argument");
    const Layout& y = h->lay; const std::string w(what);
    const RecPlan& top = h->plan[(y.L - 1) * y.D];      // the kernel-family keys speak of the TOP layer (RecPlan, sbr_common.h)
    if (w == "fused_gather") *value = h->plan[0].fuse_gather ? 1 : 0;
    else if (w == "rows_per_workgroup") *value = h->rpt;
    else if (w == "head_fused") {      // would a full batch of a training step take the one-launch head (sbr_head.hip)?  (its column chunks, or 0)
        int cc = 0, cw = 0; size_t lds = 0;
        *value = (h->sw.head_fuse && y.cfg.loss == SBR_LOSS_CCE && !simple_gemm(h) && !(y.cfg.flags & (SBR_FLAG_BF16_PROJECTION | SBR_FLAG_F32_MFMA)) &&
                  y.D == 1 && y.B == y.Bp && sbr_head_plan(y.Bp, y.N, y.HLt, &cc, &cw, &lds) && (size_t)cc * y.Bp * y.HLt <= y.ws_floats) ? cc : 0;
    }
    else if (w == "head_sampled") *value = head_sampled_taken(h, y.B) ? 1 : 0;      // a full batch of a training step: head_sampled_kernel, or the four launches
    // what the LAST step launched for the gradient of layer 0's index-input rows (-1: no step yet): 0 sorted segment reduce, 1 range form,
    // 2 segment-parallel form, 3 per-element atomics (SBR_FLAG_ATOMIC_SCATTER), 4 / 5 the overlapped tail's polling reduce / LDS-row kernel
    else if (w == "scatter_form") *value = h->last_scatter_form;
    else if (w == "step_join_gate") *value = h->last_join_gate;        // the last step's end: 1 joined by the gate on the consumers' completion words, 0 by events
    else if (w == "step_fork_gate") *value = h->last_fork_gate;        // ... its start: 1 the second side stream released by the forward chain's start word, 0 by a record
    else if (w == "tail_gate_first") *value = h->last_tail_gated;      // the last step's side stream: 1 released by the gate at its head, 0 by a record
    // what the LAST sbr_rank ran (0: none yet): its select with the row's keys in LDS (1) or streamed (2), its sort in LDS (1) or in scratch (2)
    else if (w == "rank_select") *value = h->last_rank_select;
    else if (w == "rank_sort") *value = h->last_rank_sort;
    // the LAST sbr_cluster_rank: 0 none yet, 1 only the members of each row's cluster were scored, 2 they were gathered from the full scores
    else if (w == "cluster_rank_form") *value = h->last_cluster_rank_form;
    // the LAST sbr_rank_candidates / sbr_sessions_rank_candidates: 0 none yet, 1 only the candidates were scored, 2 they were gathered from the full scores
    else if (w == "cand_rank_form") *value = h->last_cand_rank_form;
    // the kernel launches the LAST sbr_sessions_replay of any pool on this engine enqueued: 1 (0: no events, or none yet)
    else if (w == "session_replay_launches") *value = h->last_replay_launches;
    // the chunks the LAST sbr_sessions_export / sbr_sessions_import of any pool on this engine staged (0: n == 0, refused, or none yet)
    else if (w == "session_park_chunks") *value = h->last_park_chunks;
    // the LAST sbr_sessions_replay_ranks of any pool on this engine: its passes (tracing replay launches; 0: no events, or none yet), and
    // how its counting kernel read the score rows: 1 in 16-byte loads, 2 in 4-byte loads (N no multiple of 4), 0 none yet
    else if (w == "session_replay_rank_passes") *value = h->last_replay_rank_passes;
    else if (w == "session_event_rank_form") *value = h->last_event_rank_form;
    // the LAST sbr_evaluate_candidates: the same two forms (0 none yet), and the width of its last chunk's compact score matrix
    else if (w == "eval_cand_form") *value = h->last_eval_cand_form;
    else if (w == "eval_cand_lmax") *value = h->last_eval_cand_lmax;
    // the LAST sbr_evaluate_ranks: 0 none yet, 1 the row's keys stayed in LDS, 2 every pass streamed the row; and the goal items of a pass
    else if (w == "goal_rank_form") *value = h->last_goal_rank_form;
    else if (w == "goal_rank_tile") *value = kGoalRankTile;
    // the LAST sbr_evaluate_positions: 0 none yet, 1 the score row was read in 16-byte loads, 2 in 4-byte loads (N no multiple of 4)
    else if (w == "next_rank_form") *value = h->last_next_rank_form;
    else if (w == "next_rank_slots") *value = h->last_next_rank_slots;      // ... and the positions it projected per GEMM launch at the most (0 no call yet)
    // the LAST sbr_evaluate_logprob / sbr_evaluate_positions_logprob / sbr_debug_row_logprob: the same two load forms, 0 no call yet
    else if (w == "logprob_form") *value = h->last_logprob_form;
    else if (w == "row_aware_update") *value = h->last_row_aware ? 1 : 0;      // ... and whether its optimizer pass over W_in was the row-aware one
    else if (w == "cluster") *value = top.needs_fill ? 1 : 0;      // the cluster kernels (the family that wants the sentinel fill)
    else if (w == "rec_kernel") *value = top.family;               // 0 triage, 1 cluster, 2 x6p (128 units), 3 x6q (32/64), 4 other
    else if (w.rfind("rec_products_", 0) == 0 || w.rfind("rec_rows_", 0) == 0 || w.rfind("rec_workgroups_", 0) == 0) {
        // what the recurrent kernel of the top layer issues on the matrix pipe (bench.py: roofline.matrix_pipe / active_cus):
        // products = low-precision MFMA terms per f32 product (bf16x6: 6, fp16x3: 3; 0 = the exact-f32 MFMA kernels, another
        // pipe rate); rows = live batch rows among the 16 columns of an MFMA tile; workgroups = workgroups of the launch
        const bool bwd = w.size() > 4 && w.compare(w.size() - 4, 4, "_bwd") == 0;
        *value = w.rfind("rec_products_", 0) == 0 ? (bwd ? top.products_bwd : top.products_fwd)
               : w.rfind("rec_rows_", 0) == 0 ? (bwd ? top.bwd_rows : top.fwd_rows) : (bwd ? top.bwd_wgs : top.fwd_wgs);
    }
    else if (w == "tail_chunks") *value = h->tail_chunks;      // time chunks of the overlapped step tail (0: not taken)
    // ... whose consumers really run on the side streams (SBR_TAIL_OVERLAP=2 keeps them on the main stream: a data-parallel driver
    // must then not order a collective behind a side stream that produces nothing)
    else if (w == "tail_streams") *value = (h->tail_chunks >= 2 && h->sw.tail_overlap == 1) ? 1 : 0;
    else if (w == "tail_last_steps") *value = h->tail_chunks >= 2 ? h->tail_bounds.lo[1] : 0;   // time steps of chunk 0 (behind the chain)
    else if (w == "side_stream2") *value = (int64_t)(intptr_t)h->side2;
    else if (w == "tail_chain_cycles" || w == "tail_chain_ticks") {      // last overlapped-tail BPTT launch: shader cycles / 100 MHz ticks
        unsigned long long c[2] = {0, 0};
        const int nwaves = (y.Bp / h->rpt) * 8;
        SBR_HIP(hipStreamSynchronize(h->stream));
        SBR_HIP(hipMemcpy(c, (const int*)h->A(y.a_prog) + nwaves + 128, sizeof(c), hipMemcpyDeviceToHost));
        *value = (int64_t)c[w == "tail_chain_cycles" ? 0 : 1];
    }
    // overlapped tail, phase-by-phase step: the gradient ranges the two consumer streams produce (floats of the gradient section)
    else if (w == "tail_win_lo") *value = (int64_t)y.layer[0].p_Win;
    else if (w == "tail_win_hi") *value = (int64_t)y.layer[0].p_b;
    else if (w == "tail_whid_lo") *value = (int64_t)y.layer[0].p_Whid;
    else if (w == "tail_whid_hi") *value = (int64_t)y.layer[0].p_peep;
    else if (w == "arena_bytes") *value = (int64_t)(y.s_end * sizeof(float));
    else if (w == "sparse_blocks") *value = y.n_sparse;
    else if (w == "adam_table") *value = y.n_at;
    else if (w == "side_stream") *value = (int64_t)(intptr_t)h->side;
    else { sbr_set_error("unknown query '%s'", what); return SBR_EINVAL; }
    return SBR_OK;
}

extern "C" int sbr_enable_timing(sbr_handle* h, int on) {
    CHECK_ARG(h, "null handle");
    if (on)
        for (int r = 0; r < sbr_handle::kRing; ++r)
            for (int i = 0; i < SBR_N_PHASES; ++i) if (!h->ev[r][i]) SBR_HIP(hipEventCreate(&h->ev[r][i]));
    CHECK_ARG(on >= 0 && on <= SBR_N_PHASES, "on = %d: 0 off, 1 every phase, 2 + p only phase p", on);
    h->timing = on != 0; h->ring_used = 0; h->ring_cur = 0;
    h->timing_marks = on == 1 ? 0xffu : on >= 2 ? (3u << (on - 2)) : 0u;      // a phase lies between marks p and p + 1
    return SBR_OK;
}

// Chain-only timing: on = 1 starts collecting an event pair around every launch of a recurrent chain kernel (all layers, both
// directions; up to 256 launches), on = 0 stops and reports.  us[0] / us[1]: device time summed over the forward / backward chain
// launches since the start; n[0] / n[1]: how many launches that was (divide by the steps run in between).  A survey facility
// like sbr_enable_timing(h, 1): the records cost the stream a few microseconds each.
extern "C" int sbr_chain_times(sbr_handle* h, int on, float us[2], int n[2]) {
    CHECK_ARG(h, "null handle");
    if (on) { h->ch_n = 0; h->chain_timing = true; return SBR_OK; }
    CHECK_ARG(us && n, "null argument");
    h->chain_timing = false;
    SBR_HIP(hipDeviceSynchronize());
    us[0] = us[1] = 0.f; n[0] = n[1] = 0;
    for (int r = 0; r < h->ch_n; ++r) {
        float ms = 0.f;
        if (!h->ev_ch[r][0] || !h->ev_ch[r][1] || hipEventElapsedTime(&ms, h->ev_ch[r][0], h->ev_ch[r][1]) != hipSuccess) continue;
        us[h->ch_dir[r] & 1] += ms * 1000.f; n[h->ch_dir[r] & 1] += 1;
    }
    h->ch_n = 0;
    return SBR_OK;
}

// mean over the (up to 64 most recent) train steps recorded since sbr_enable_timing(h, 1)
extern "C" int sbr_phase_times(sbr_handle* h, float us[SBR_N_PHASES]) {
    CHECK_ARG(h && us, "null argument");
    if (!h->timing || h->ring_used == 0) { sbr_set_error("no timed train step recorded"); return SBR_ESTATE; }
    SBR_HIP(hipStreamSynchronize(h->stream));
    const int n = std::min(h->ring_used, (int)sbr_handle::kRing);
    for (int i = 0; i < SBR_N_PHASES; ++i) us[i] = 0.f;
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < SBR_N_PHASES - 1; ++i) {
            float ms = 0.f;
            if (((h->timing_marks >> i) & 3) != 3) continue;          // this phase was not bracketed
            if (hipEventElapsedTime(&ms, h->ev[r][i], h->ev[r][i + 1]) != hipSuccess) ms = 0.f;
            us[i] += ms * 1000.f / n;
        }
    for (int i = 0; i < SBR_N_PHASES - 1; ++i) us[SBR_N_PHASES - 1] += us[i];
    return SBR_OK;
}
