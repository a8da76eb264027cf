// The ranking and evaluation calls of the C-ABI (include/sbr_rnn.h): sbr_topk, sbr_rank, sbr_evaluate, sbr_evaluate_ranks,
// sbr_evaluate_positions, sbr_evaluate_logprob, sbr_evaluate_positions_logprob, sbr_evaluate_candidates, sbr_cluster_rank, sbr_cluster_evaluate, sbr_rank_candidates, sbr_sessions_rank_candidates.
// Host code only (kernels: sbr_rank.hip, sbr_eval.hip, sbr_eval_cand.hip, sbr_cluster_rank.hip, sbr_cand_rank.hip, sbr_cluster_eval.hip; forward pass and projection:
// sbr_api.hip), built from the shared pieces below: scores, ONE exclusion launch per ranking (launch_exclude: what
// is excluded is an ExclSources, where it lands an ExclCatalogue or ExclCluster, sbr_device.h), select and sort (rank_rows).
// Every call waits for the device once, in check_fault.
#include "sbr_common.h"
#include "sbr_device.h"
#include <algorithm>

// The scratch of these calls -- the device copies of the lists, the selected (key, id) pairs, the radix sort's second pair, the
// results -- is the handle's own allocation and not part of the arena: its size follows k and the lists.
static int rank_scratch(sbr_handle* h, size_t bytes) {
    if (bytes <= h->rank_scratch_bytes) return SBR_OK;
    if (h->rank_scratch) { (void)hipFree(h->rank_scratch); h->rank_scratch = nullptr; h->rank_scratch_bytes = 0; }
    if (hipMalloc(&h->rank_scratch, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->rank_scratch = nullptr;
        sbr_set_error("sbr_rank: hipMalloc(%zu) of the ranking scratch failed", bytes);
        return SBR_ENOMEM;
    }
    h->rank_scratch_bytes = bytes;
    return SBR_OK;
}

// byte offsets into the scratch, every region on a 256-byte boundary; `at` ends as the size to allocate
struct Carver {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; }
};

// what select + sort of `rows` rows to `depth` places work in: the selected count, the (key, id) pairs and, with radix, the second pair
struct RankWork { size_t nsel, k0, i0, k1, i1; };
static RankWork carve_rank_work(Carver& cv, int rows, int depth, bool radix) {
    const size_t n = (size_t)rows * depth;
    RankWork w;
    w.nsel = cv.take((size_t)rows * sizeof(int));
    w.k0 = cv.take(n * sizeof(unsigned)); w.i0 = cv.take(n * sizeof(int));
    w.k1 = cv.take(radix ? n * sizeof(unsigned) : 0); w.i1 = cv.take(radix ? n * sizeof(int) : 0);
    return w;
}

// the ordered top `depth` of every row of scores [rows][width] into out_ids / out_scores [rows][depth]
static int rank_rows(sbr_handle* h, char* S, const RankWork& w, const float* scores, int rows, int width, int depth, int* out_ids, float* out_scores) {
    SBR_LAUNCH(launch_rank_select(h->stream, scores, rows, width, depth, (unsigned*)(S + w.k0), (int*)(S + w.i0), (int*)(S + w.nsel), &h->last_rank_select));
    SBR_LAUNCH(launch_rank_sort(h->stream, scores, rows, width, depth, (unsigned*)(S + w.k0), (int*)(S + w.i0), (unsigned*)(S + w.k1), (int*)(S + w.i1),
                                (const int*)(S + w.nsel), out_ids, out_scores, &h->last_rank_sort));
    return SBR_OK;
}

// The per-row exclusion lists of sbr_rank and sbr_cluster_rank: the caller's CSR, and where its device copy sits in the scratch
struct ExclLists {
    const int32_t* ids; const int64_t* off; int rows; int64_t n;      // n: ids in all
    size_t o_off, o_ids;
    const long long* dev_off(const char* S) const { return off ? (const long long*)(S + o_off) : nullptr; }
    const int* dev_ids(const char* S) const { return off ? (const int*)(S + o_ids) : nullptr; }
};
// everything about the lists is checked here, before anything is launched
static int excl_check(const int32_t* excl_ids, const int64_t* excl_off, int rows, int N, ExclLists& x) {
    CHECK_ARG((excl_ids == nullptr) == (excl_off == nullptr), "excl_ids and excl_off: both or neither");
    x = ExclLists{excl_ids, excl_off, rows, 0, 0, 0};
    if (!excl_off) return SBR_OK;
    CHECK_ARG(excl_off[0] >= 0, "excl_off[0] = %lld is negative", (long long)excl_off[0]);
    for (int r = 0; r < rows; ++r)
        CHECK_ARG(excl_off[r + 1] >= excl_off[r], "excl_off decreases at row %d (%lld -> %lld)", r, (long long)excl_off[r], (long long)excl_off[r + 1]);
    for (int64_t j = excl_off[0]; j < excl_off[rows]; ++j)
        CHECK_ARG(excl_ids[j] >= 0 && excl_ids[j] < N, "excluded id %d outside [0,%d)", excl_ids[j], N);
    x.n = excl_off[rows] - excl_off[0];
    return SBR_OK;
}
static void excl_carve(Carver& cv, ExclLists& x) {
    x.o_off = cv.take((size_t)(x.rows + 1) * sizeof(long long)); x.o_ids = cv.take((size_t)x.n * sizeof(int));
}
static int excl_upload(sbr_handle* h, char* S, const ExclLists& x) {
    if (!x.off) return SBR_OK;
    std::vector<long long> off((size_t)x.rows + 1);
    for (int r = 0; r <= x.rows; ++r) off[r] = (long long)(x.off[r] - x.off[0]);
    // (pageable host memory: both copies have left the host buffers when they return)
    SBR_HIP(hipMemcpyAsync(S + x.o_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    if (x.n) SBR_HIP(hipMemcpyAsync(S + x.o_ids, x.ids + x.off[0], (size_t)x.n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));           // `off` goes out of scope
    return SBR_OK;
}

// what sbr_rank and sbr_cluster_rank exclude from a row: its uploaded list and, when asked, its input window
static ExclSources excl_sources(const sbr_handle* h, const char* S, const ExclLists& x, int exclude_input) {
    ExclSources src;
    src.lists(x.dev_ids(S), x.dev_off(S));
    if (exclude_input) src.window(h->bX, h->blen, h->lay.T, h->lay.F);
    return src;
}

// the hidden state of the current batch with every output row current: full_scores minus its projection
int forward_current(sbr_handle* h) {
    int rc;
    if (!h->fwd_done && (rc = sbr_forward(h)) != SBR_OK) return rc;
    return flush_lazy(h, 1);      // the sampled heads step W_out^T / b_out rows lazily: every row that is scored must be current
}

// The compiled test function's ranking (rnn_base.py:196-211), the oldest call: a second entry to sbr_rank's pipeline with its own
// contract -- k <= 64, the result in the arena's a_topk (the Layout keeps the buffer, so every arena offset is what it was), and
// exclude_seen in place of the lists.  Softmax is monotone: ranking the biased logits == ranking softmax(logits) * (1 - exclude)
// (:200-207) whenever at least k items are not excluded.
// Against the k arg-max passes this call used to run, the ids are the same (tests/test_gpu_rank.py) and three things differ: the
// score row is no longer overwritten with -inf at the winners; an id outside [0, N) in a device-resident batch is skipped where it
// used to be written through; and sbr_query "rank_select" / "rank_sort" now also tell what an sbr_topk call ran.
extern "C" int sbr_topk(sbr_handle* h, int k, int exclude_seen, int32_t* ids_host) {
    CHECK_ARG(h && ids_host, "null argument");
    if (!h->have_batch) { sbr_set_error("sbr_topk: no batch set"); return SBR_ESTATE; }
    const Layout& y = h->lay;
    const int rows = h->n_rows;
    CHECK_ARG(k >= 1 && k <= 64 && k <= y.N, "k=%d outside [1,min(64,N)]", k);
    Carver cv;
    const RankWork w = carve_rank_work(cv, rows, k, k > kRankSortLds);
    const size_t o_osc = cv.take((size_t)rows * k * sizeof(float));
    int rc;
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    if ((rc = full_scores(h, 0)) != SBR_OK) return rc;
    float* lg = h->A(y.a_logits);
    // exclude_seen 1: viewed items can never be ranked (top_k_recommendations, rnn_base.py:154-155); 2: the compiled test
    // function's scores * (1 - exclude) (:201-202) -- the same ranking for probabilities, NOT for RNNMargin's raw outputs,
    // where a viewed item then scores 0 and outranks every negative one
    ExclSources seen;
    if (exclude_seen) seen.window(h->bX, h->blen, y.T, y.F);
    const float value = (exclude_seen == 2 && SBR_LOSS_IS_MARGIN(y.cfg.loss)) ? 0.0f : -INFINITY;
    SBR_LAUNCH(launch_exclude(h->stream, rows, seen, ExclCatalogue{lg, y.N, value}));
    int* ids = (int*)h->A(y.a_topk);
    if ((rc = rank_rows(h, S, w, lg, rows, y.N, k, ids, (float*)(S + o_osc))) != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(ids_host, ids, (size_t)rows * k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return check_fault(h);          // a forward that gave up must not hand out rankings (test.py, validation)
}

// Ordered top-k of any depth with per-row exclusion lists (top_k_recommendations' k and exclude=, rnn_base.py:140-165, for a
// whole batch): sbr_rank.hip.
extern "C" int sbr_rank(sbr_handle* h, int k, int exclude_input, const int32_t* excl_ids, const int64_t* excl_off,
                        int32_t* ids_host, float* scores_host) {
    CHECK_ARG(h && ids_host, "null argument");
    if (!h->have_batch) { sbr_set_error("sbr_rank: no batch set"); return SBR_ESTATE; }
    const Layout& y = h->lay;
    const int rows = h->n_rows;
    CHECK_ARG(k >= 1 && k <= y.N, "k=%d outside [1,N=%d]", k, y.N);
    ExclLists x;
    int rc;
    if ((rc = excl_check(excl_ids, excl_off, rows, y.N, x)) != SBR_OK) return rc;
    const size_t rk = (size_t)rows * k;
    Carver cv;
    excl_carve(cv, x);
    const RankWork w = carve_rank_work(cv, rows, k, k > kRankSortLds);
    const size_t o_oid = cv.take(rk * sizeof(int)), o_osc = cv.take(rk * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    if ((rc = full_scores(h, 0)) != SBR_OK) return rc;      // the very floats sbr_topk ranks (and flushes lazily stepped rows)
    float* lg = h->A(y.a_logits);
    if ((rc = excl_upload(h, S, x)) != SBR_OK) return rc;
    SBR_LAUNCH(launch_exclude(h->stream, rows, excl_sources(h, S, x, exclude_input), ExclCatalogue{lg, y.N, -INFINITY}));
    if ((rc = rank_rows(h, S, w, lg, rows, y.N, k, (int*)(S + o_oid), (float*)(S + o_osc))) != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(ids_host, S + o_oid, rk * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (scores_host) SBR_HIP(hipMemcpyAsync(scores_host, S + o_osc, rk * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return check_fault(h);          // a forward that gave up must not hand out rankings
}

// The next-item ranking of kept session states (include/sbr_rnn.h "Stateful sessions"; the pool and its step: sbr_session.hip):
// sbr_rank's pipeline on rows that come from the pool instead of a forward pass.  Per chunk of local_batch rows (a_logits holds Bp
// rows): the top layer's current states of the chunk's slots gathered into a contiguous [rows][HLt] matrix -> project_rows ->
// launch_exclude (the caller's lists and the slots' history rings, ExclSources::sessions) -> rank_rows.  have_batch / fwd_done and the
// batch buffers are not touched.  The call waits once, in check_fault.
extern "C" int sbr_sessions_rank(sbr_sessions* ses, const int32_t* slots, int64_t n, int k, int exclude_mode, const int32_t* excl_ids,
                                 const int64_t* excl_off, int32_t* ids_host, float* scores_host) {
    CHECK_ARG(ses && slots && ids_host, "null argument");
    sbr_handle* h = ses->h;
    const Layout& y = h->lay;
    const SesPool& p = ses->p;
    int rc;
    if ((rc = sessions_state_check(ses, "sbr_sessions_rank")) != SBR_OK) return rc;
    CHECK_ARG(n >= 1 && n <= 0x7fffffff, "sbr_sessions_rank: n=%lld sessions: at least one", (long long)n);
    CHECK_ARG(k >= 1 && k <= y.N, "k=%d outside [1,N=%d]", k, y.N);
    CHECK_ARG(exclude_mode >= SBR_SESSION_EXCL_NONE && exclude_mode <= SBR_SESSION_EXCL_HISTORY, "unknown exclusion mode %d", exclude_mode);
    if ((rc = sessions_check_slots(ses, "sbr_sessions_rank", slots, n, false)) != SBR_OK) return rc;
    ExclLists x;
    if ((rc = excl_check(excl_ids, excl_off, (int)n, y.N, x)) != SBR_OK) return rc;
    const int B = y.B;
    const size_t nk = (size_t)n * k;
    Carver cv;
    const size_t o_slots = cv.take((size_t)n * sizeof(int));
    excl_carve(cv, x);
    const size_t o_states = cv.take((size_t)B * y.HLt * sizeof(float));
    const RankWork w = carve_rank_work(cv, B, k, k > kRankSortLds);
    const size_t o_oid = cv.take(nk * sizeof(int)), o_osc = cv.take(nk * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    if ((rc = flush_lazy(h, 1)) != SBR_OK) return rc;      // every item is scored: all of W_out^T / b_out must be current (forward_current's flush)
    // (pageable host memory: the copy has left the caller's array when it returns)
    SBR_HIP(hipMemcpyAsync(S + o_slots, slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if ((rc = excl_upload(h, S, x)) != SBR_OK) return rc;
    const int* dslots = (const int*)(S + o_slots);
    float* states = (float*)(S + o_states);
    float* lg = h->A(y.a_logits);
    for (int64_t c0 = 0; c0 < n; c0 += B) {
        const int rows = (int)std::min<int64_t>(B, n - c0);
        SBR_LAUNCH(launch_ses_gather_top(s, p, dslots + c0, rows, states));
        if ((rc = project_rows(h, states, rows, lg, 0)) != SBR_OK) return rc;      // the floats sbr_rank ranks for a row in that state
        ExclSources src;
        if (x.off) src.lists(x.dev_ids(S), x.dev_off(S) + c0);
        src.sessions(dslots + c0, p.ring, p.events, p.ring_len, p.history, exclude_mode);
        SBR_LAUNCH(launch_exclude(s, rows, src, ExclCatalogue{lg, y.N, -INFINITY}));
        if ((rc = rank_rows(h, S, w, lg, rows, y.N, k, (int*)(S + o_oid) + (size_t)c0 * k, (float*)(S + o_osc) + (size_t)c0 * k)) != SBR_OK) return rc;
    }
    SBR_HIP(hipMemcpyAsync(ids_host, S + o_oid, nk * sizeof(int), hipMemcpyDeviceToHost, s));
    if (scores_host) SBR_HIP(hipMemcpyAsync(scores_host, S + o_osc, nk * sizeof(float), hipMemcpyDeviceToHost, s));
    return check_fault(h);
}

// sbr_sessions_replay that also ranks every event before it is fed (include/sbr_rnn.h "Stateful sessions").  The call
// is cut in time into passes, all planned on the host before the first launch: a pass takes the rows that still have events, at
// most P events each, P the largest for which the pass's (row, event) pairs stay within group_rows (P = 1 where the rows alone
// exceed it), longest first.  Per pass: ONE tracing replay launch from the kept state (launch_ses_replay_rows: the replay itself, which
// also writes the top layer's state in front of every event into `trace`), then per group of at most group_rows trace rows
// project_rows -- the floats sbr_sessions_rank projects for a slot in that state -- and ses_event_rank_kernel.  The replay's commit
// overwrites event counts and rings, so those of the named slots are kept aside first (launch_ses_keep).  Everything on the engine's
// stream without a host wait; the call waits once, in check_fault.  Rows, trace, scores, what is kept aside and the results live in
// the handle's ranking scratch; the events in the pool's buffers, as for replay.
extern "C" int sbr_sessions_replay_ranks(sbr_sessions* ses, const int32_t* slots, int64_t n, const int32_t* items, const int32_t* second,
                                         const int64_t* off, int exclude_mode, int64_t group_rows, int32_t* ranks_host,
                                         int32_t* n_rankable_host, int64_t* events_before_host) {
    static const char* const call = "sbr_sessions_replay_ranks";
    CHECK_ARG(ses, "null argument");
    sbr_handle* h = ses->h;
    const Layout& y = h->lay;
    const SesPool& p = ses->p;
    int rc;
    if ((rc = sessions_state_check(ses, call)) != SBR_OK) return rc;
    CHECK_ARG(exclude_mode >= SBR_SESSION_EXCL_NONE && exclude_mode <= SBR_SESSION_EXCL_HISTORY, "%s: unknown exclusion mode %d", call, exclude_mode);
    CHECK_ARG(group_rows >= 0, "%s: group_rows=%lld is negative", call, (long long)group_rows);
    if ((rc = ses_replay_check(ses, call, slots, n, items, second, off)) != SBR_OK) return rc;
    const int64_t total = n ? off[n] : 0;
    CHECK_ARG(total == 0 || (ranks_host && n_rankable_host), "%s: ranks_host and n_rankable_host are required (%lld events)", call, (long long)total);
    CHECK_ARG(total <= 0x7fffffff, "%s: %lld events in one call, at most 2^31 - 1", call, (long long)total);
    h->last_replay_rank_passes = 0;
    if (n == 0 || (total == 0 && !events_before_host)) return SBR_OK;
    const int64_t G = group_rows ? group_rows : (int64_t)std::max<size_t>(1, kNextRankScoreBytes / ((size_t)y.N * sizeof(float)));
    // --- the passes
    struct Left { int64_t at, left; int row; };                       // a row of the call: its next event, how many are left
    std::vector<Left> left;
    for (int64_t r = 0; r < n; ++r)
        if (off[r + 1] > off[r]) left.push_back(Left{off[r], off[r + 1] - off[r], (int)r});
    std::vector<SesRow> rows;                                         // the rows of every pass, one pass behind the other
    std::vector<SesTraceRow> trows;
    std::vector<size_t> pass_at;                                      // where a pass starts in rows (and, at the end, rows.size())
    std::vector<int64_t> pass_trace;                                  // its trace rows
    int64_t max_trace = 0;
    while (!left.empty()) {
        auto pairs = [&](int64_t P) { int64_t sum = 0; for (const Left& l : left) sum += std::min(l.left, P); return sum; };
        int64_t P = 1, hi = 0;
        for (const Left& l : left) hi = std::max(hi, l.left);
        while (P < hi) {                                              // the largest P in [1, hi] whose pairs fit G (1 if none does)
            const int64_t mid = P + (hi - P + 1) / 2;
            if (pairs(mid) <= G) P = mid; else hi = mid - 1;
        }
        const size_t r0 = rows.size();
        pass_at.push_back(r0);
        for (const Left& l : left) rows.push_back(SesRow{l.at, std::min(l.left, P), slots[l.row]});
        // longest first (stable): a tile's rows end together; the trace rows follow that order
        std::vector<size_t> order(left.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return rows[r0 + a].len > rows[r0 + b].len; });
        std::vector<SesRow> sorted(order.size());
        int64_t at = 0;
        for (size_t i = 0; i < order.size(); ++i) {
            sorted[i] = rows[r0 + order[i]];
            const int row = left[order[i]].row;
            trows.push_back(SesTraceRow{at, off[row], row});
            at += sorted[i].len;
        }
        std::copy(sorted.begin(), sorted.end(), rows.begin() + r0);
        pass_trace.push_back(at);
        max_trace = std::max(max_trace, at);
        std::vector<Left> next;
        for (const Left& l : left) { const int64_t k = std::min(l.left, P); if (l.left > k) next.push_back(Left{l.at + k, l.left - k, l.row}); }
        left.swap(next);
    }
    pass_at.push_back(rows.size());
    // --- the scratch
    const LayerLayout& top = y.layer[y.L - 1];
    const int64_t score_rows = std::min(G, max_trace);
    Carver cv;
    const size_t o_slots = cv.take((size_t)n * sizeof(int)), o_e0 = cv.take((size_t)n * sizeof(long long));
    const size_t o_ring = cv.take(total ? (size_t)n * p.ring_len * sizeof(int) : 0);
    const size_t o_rows = cv.take(rows.size() * sizeof(SesRow)), o_trows = cv.take(trows.size() * sizeof(SesTraceRow));
    const size_t o_ranks = cv.take((size_t)total * sizeof(int)), o_nrk = cv.take((size_t)total * sizeof(int));
    const size_t o_trace = cv.take((size_t)max_trace * top.Hp * sizeof(float));
    const size_t o_scores = cv.take((size_t)score_rows * y.N * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    // lazily stepped rows: the index-input block as for replay (ses_replay_events), the output rows as for rank
    if (total) {
        if ((rc = ses_replay_events(ses, call, items, second, total)) != SBR_OK) return rc;
        if ((rc = flush_lazy(h, 1)) != SBR_OK) return rc;
    }
    // (pageable host memory: the copies have left the host arrays when they return)
    SBR_HIP(hipMemcpyAsync(S + o_slots, slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    SBR_LAUNCH(launch_ses_keep(s, p, (const int*)(S + o_slots), n, (long long*)(S + o_e0), total ? (int*)(S + o_ring) : nullptr));
    if (total) {
        SBR_HIP(hipMemcpyAsync(S + o_rows, rows.data(), rows.size() * sizeof(SesRow), hipMemcpyHostToDevice, s));
        SBR_HIP(hipMemcpyAsync(S + o_trows, trows.data(), trows.size() * sizeof(SesTraceRow), hipMemcpyHostToDevice, s));
    }
    float* trace = (float*)(S + o_trace);
    float* scores = (float*)(S + o_scores);
    for (size_t ps = 0; ps + 1 < pass_at.size(); ++ps) {
        const SesRow* drows = (const SesRow*)(S + o_rows) + pass_at[ps];
        const SesTraceRow* dtrows = (const SesTraceRow*)(S + o_trows) + pass_at[ps];
        const int n_rows = (int)(pass_at[ps + 1] - pass_at[ps]);
        SBR_LAUNCH(launch_ses_replay_rows(ses, drows, n_rows, second != nullptr, dtrows, trace));
        for (int64_t g0 = 0; g0 < pass_trace[ps]; g0 += score_rows) {
            const int gr = (int)std::min<int64_t>(score_rows, pass_trace[ps] - g0);
            if ((rc = project_rows(h, trace + (size_t)g0 * top.Hp, gr, scores, 0)) != SBR_OK) return rc;
            const SesEventRank a{drows, dtrows, n_rows, ses->d_ev_items, (const long long*)(S + o_e0), (const int*)(S + o_ring), p.ring_len, p.history,
                                 exclude_mode, g0, scores, y.N, (int*)(S + o_ranks), (int*)(S + o_nrk)};
            SBR_LAUNCH(launch_ses_event_rank(s, a, gr, &h->last_event_rank_form));
        }
    }
    h->last_replay_rank_passes = (int)pass_trace.size();
    if (total) {
        SBR_HIP(hipMemcpyAsync(ranks_host, S + o_ranks, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
        SBR_HIP(hipMemcpyAsync(n_rankable_host, S + o_nrk, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "the event counts are fetched as they are");
    if (events_before_host) SBR_HIP(hipMemcpyAsync(events_before_host, S + o_e0, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, s));
    return check_fault(h);          // the call's one wait for the device
}

// ---------------------------------------------------------------------------------------
// Ranking inside a candidate list the caller brings (include/sbr_rnn.h: sbr_rank_candidates, sbr_sessions_rank_candidates; kernels
// and the accumulation-order argument: sbr_cand_rank.hip, sbr_cluster_rank.hip)
// ---------------------------------------------------------------------------------------
// The caller's candidate lists, a CSR over the rows of the call (shared: ONE list for every row), and where their device copy sits in
// the scratch: the offsets as int rebased to 0 and, behind them, what makes the lists "clusters" for the shared pieces -- the cluster
// of a row (its own index, or 0 for the shared list) and, for the shared list, crk_score_kernel's tile tables for a full chunk of rows
// and for the last, shorter one
struct CandLists {
    const int32_t* ids; const int64_t* off; int64_t rows; bool shared; int64_t n;      // n: ids in all
    int chunk, last;                                     // rows of a full chunk of the call and of its last one
    size_t o_meta, o_ids, w_csel, w_full, w_last, words; // offsets in the scratch (bytes) and inside the meta words
    const int* dev_off(const char* S) const { return (const int*)(S + o_meta); }
    const int* dev_csel(const char* S) const { return (const int*)(S + o_meta) + w_csel; }
    const int* dev_work(const char* S, int n_rows) const { return (const int*)(S + o_meta) + (n_rows == chunk ? w_full : w_last); }
    const int* dev_ids(const char* S) const { return (const int*)(S + o_ids); }
    int64_t lists() const { return shared ? 1 : rows; }
    // the width of the compact matrix of rows [c0, c0 + n_rows): their longest list, rounded up to 4 as the cluster road's
    int lmax(int64_t c0, int n_rows) const {
        int64_t longest = 0;
        if (shared) longest = off[1] - off[0];
        else for (int64_t r = c0; r < c0 + n_rows; ++r) longest = std::max<int64_t>(longest, off[r + 1] - off[r]);
        return (int)std::max<int64_t>(4, (longest + 3) / 4 * 4);
    }
};
// everything about the lists is checked here, before anything is launched; chunk: rows of the call that are ranked together
static int cand_check(const int32_t* cand_ids, const int64_t* cand_off, int64_t rows, int chunk, int shared, int N, CandLists& c) {
    CHECK_ARG(cand_ids && cand_off, "cand_ids and cand_off: both are required");
    CHECK_ARG(rows >= 1, "no rows to rank");
    c = CandLists{cand_ids, cand_off, rows, shared != 0, 0, (int)std::min<int64_t>(rows, chunk), 0, 0, 0, 0, 0, 0, 0};      // (rows >= 1)
    c.last = rows % c.chunk ? (int)(rows % c.chunk) : c.chunk;
    const int64_t nl = c.lists();
    CHECK_ARG(cand_off[0] >= 0, "cand_off[0] = %lld is negative", (long long)cand_off[0]);
    for (int64_t r = 0; r < nl; ++r)
        CHECK_ARG(cand_off[r + 1] >= cand_off[r], "cand_off decreases at row %lld (%lld -> %lld)", (long long)r, (long long)cand_off[r], (long long)cand_off[r + 1]);
    c.n = cand_off[nl] - cand_off[0];
    for (int64_t r = 0; r < nl; ++r) {
        // a pass without branches first (the compiler vectorises it: a third of the time of the walk below, and the lists of a call can
        // hold millions of ids); only a list that fails is walked again, for the offender
        const int32_t* l = cand_ids + cand_off[r];
        const int64_t len = cand_off[r + 1] - cand_off[r];
        unsigned bad = 0;
        for (int64_t j = 0; j < len; ++j) bad |= (unsigned)((unsigned)l[j] >= (unsigned)N);
        for (int64_t j = 1; j < len; ++j) bad |= (unsigned)(l[j - 1] >= l[j]);
        if (!bad) continue;
        for (int64_t j = cand_off[r]; j < cand_off[r + 1]; ++j) {
            const int id = cand_ids[j];
            CHECK_ARG(id >= 0 && id < N, "candidate %d of row %lld, at position %lld of its list, is outside [0,%d)", id, (long long)r, (long long)(j - cand_off[r]), N);
            CHECK_ARG(j == cand_off[r] || cand_ids[j - 1] < id, "the candidates of row %lld are not strictly ascending at position %lld (%d after %d)",
                      (long long)r, (long long)(j - cand_off[r]), id, cand_ids[j - 1]);
        }
    }
    CHECK_ARG(c.n <= 0x7fffffff, "the candidate lists of one call hold %lld ids, at most 2^31 - 1", (long long)c.n);
    return SBR_OK;
}
static void cand_carve(Carver& cv, CandLists& c) {
    c.w_csel = (size_t)c.lists() + 1;
    c.w_full = c.w_csel + c.chunk;
    c.w_last = c.w_full + (c.shared ? sbr_crk_group_words(c.chunk, 1) : 0);
    c.words = c.w_last + (c.shared && c.last != c.chunk ? sbr_crk_group_words(c.last, 1) : 0);
    c.o_meta = cv.take(c.words * sizeof(int)); c.o_ids = cv.take((size_t)c.n * sizeof(int));
}
// (excl_upload's pattern: two asynchronous copies, one wait)
static int cand_upload(sbr_handle* h, char* S, const CandLists& c) {
    std::vector<int> meta(c.words);
    for (int64_t r = 0; r <= c.lists(); ++r) meta[r] = (int)(c.off[r] - c.off[0]);
    for (int r = 0; r < c.chunk; ++r) meta[c.w_csel + r] = c.shared ? 0 : r;
    if (c.shared) {
        cand_shared_work(c.chunk, meta.data() + c.w_full);
        if (c.last != c.chunk) cand_shared_work(c.last, meta.data() + c.w_last);
    }
    // (pageable host memory: both copies have left the host buffers when they return)
    SBR_HIP(hipMemcpyAsync(S + c.o_meta, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (c.n) SBR_HIP(hipMemcpyAsync(S + c.o_ids, c.ids + c.off[0], (size_t)c.n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    SBR_HIP(hipStreamSynchronize(h->stream));           // `meta` goes out of scope
    return SBR_OK;
}

// form 1 restates the exact-f32 projection for the candidates only; the bf16 and the triage projections round differently, and their
// scores are gathered from the matrix those kernels write (form 2, also SBR_CAND_RANK=0)
static bool cand_rank_restricted(const sbr_handle* h) {
    return h->sw.cand_rank && !(h->lay.cfg.flags & SBR_FLAG_BF16_PROJECTION) && !simple_gemm(h);
}

// what a chunk of a candidate ranking works in beside the lists: the compact score matrix, select + sort, the ranked places
struct CandWork { size_t cs; RankWork w; size_t pos, psc; };
static CandWork carve_cand_work(Carver& cv, const CandLists& c, int k) {
    int lmax = 4;
    for (int64_t c0 = 0; c0 < c.rows; c0 += c.chunk) lmax = std::max(lmax, c.lmax(c0, (int)std::min<int64_t>(c.chunk, c.rows - c0)));
    const int kk = std::min(k, lmax);
    CandWork cw;
    cw.cs = cv.take((size_t)c.chunk * lmax * sizeof(float));
    cw.w = carve_rank_work(cv, c.chunk, kk, kk > kRankSortLds);
    cw.pos = cv.take((size_t)c.chunk * kk * sizeof(int)); cw.psc = cv.take((size_t)c.chunk * kk * sizeof(float));
    return cw;
}

// Rows [c0, c0 + rows) of the call: the candidates' scores into cs [rows][lmax] -- scored from `states` [rows][HLt] (restricted: the
// shared list by crk_score_kernel as one cluster of all rows, per-row lists by cand_score_kernel) or gathered from the full scores `lg`
// [rows][N] --, then sbr_cluster_rank's pipeline with the row's own list as its cluster: exclusion, select and sort to
// min(k, lmax) places, places -> ids.
static int cand_rank_chunk(sbr_handle* h, char* S, const CandLists& c, const CandWork& cw, const float* states, const float* lg, int64_t c0,
                           int rows, const ExclSources& src, int k, bool restricted, int* out_ids, float* out_scores) {
    const Layout& y = h->lay;
    hipStream_t s = h->stream;
    const int lmax = c.lmax(c0, rows), kk = std::min(k, lmax), C = c.shared ? 1 : rows;
    const int* moff = c.dev_off(S) + (c.shared ? 0 : c0);
    const int* csel = c.dev_csel(S);
    const int* mem = c.dev_ids(S);
    float* cs = (float*)(S + cw.cs);
    if (!restricted)
        SBR_LAUNCH(launch_crk_gather(s, lg, y.N, csel, mem, moff, rows, lmax, cs));
    else if (c.shared)
        SBR_LAUNCH(launch_crk_score(s, states, y.HLt, h->P(y.p_WoutT), h->P(y.p_bout), y.HLt, mem, moff, c.dev_work(S, rows), rows, 1, lmax, cs));
    else
        SBR_LAUNCH(launch_cand_score(s, states, y.HLt, h->P(y.p_WoutT), h->P(y.p_bout), y.HLt, mem, moff, rows, lmax, cs));
    h->last_cand_rank_form = restricted ? 1 : 2;
    SBR_LAUNCH(launch_exclude(s, rows, src, ExclCluster{cs, lmax, csel, C, mem, moff, y.N}));
    int rc;
    if ((rc = rank_rows(h, S, cw.w, cs, rows, lmax, kk, (int*)(S + cw.pos), (float*)(S + cw.psc))) != SBR_OK) return rc;
    SBR_LAUNCH(launch_crk_translate(s, (const int*)(S + cw.pos), (const float*)(S + cw.psc), kk, k, csel, mem, moff, rows, out_ids, out_scores, nullptr));
    return SBR_OK;
}

// sbr_rank restricted to each row's candidate list
extern "C" int sbr_rank_candidates(sbr_handle* h, int k, const int32_t* cand_ids, const int64_t* cand_off, int shared, int exclude_input,
                                   const int32_t* excl_ids, const int64_t* excl_off, int32_t* ids_host, float* scores_host) {
    CHECK_ARG(h && ids_host, "null argument");
    if (!h->have_batch) { sbr_set_error("sbr_rank_candidates: no batch set"); return SBR_ESTATE; }
    const Layout& y = h->lay;
    const int rows = h->n_rows;
    CHECK_ARG(k >= 1 && k <= y.N, "k=%d outside [1,N=%d]", k, y.N);
    CandLists c;
    ExclLists x;
    int rc;
    if ((rc = cand_check(cand_ids, cand_off, rows, rows, shared, y.N, c)) != SBR_OK) return rc;
    if ((rc = excl_check(excl_ids, excl_off, rows, y.N, x)) != SBR_OK) return rc;
    const size_t rk = (size_t)rows * k;
    Carver cv;
    excl_carve(cv, x);
    cand_carve(cv, c);
    const CandWork cw = carve_cand_work(cv, c, k);
    const size_t o_oid = cv.take(rk * sizeof(int)), o_osc = cv.take(rk * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    const bool restricted = cand_rank_restricted(h);
    if ((rc = restricted ? forward_current(h) : full_scores(h, 0)) != SBR_OK) return rc;
    if ((rc = excl_upload(h, S, x)) != SBR_OK || (rc = cand_upload(h, S, c)) != SBR_OK) return rc;
    if ((rc = cand_rank_chunk(h, S, c, cw, h_last(h), h->A(y.a_logits), 0, rows, excl_sources(h, S, x, exclude_input), k, restricted,
                              (int*)(S + o_oid), (float*)(S + o_osc))) != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(ids_host, S + o_oid, rk * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (scores_host) SBR_HIP(hipMemcpyAsync(scores_host, S + o_osc, rk * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return check_fault(h);          // a forward that gave up must not hand out rankings
}

// sbr_sessions_rank restricted to each named slot's candidate list: its chunks, its exclusion sources, cand_rank_chunk per chunk
extern "C" int sbr_sessions_rank_candidates(sbr_sessions* ses, const int32_t* slots, int64_t n, int k, const int32_t* cand_ids,
                                            const int64_t* cand_off, int shared, int exclude_mode, const int32_t* excl_ids,
                                            const int64_t* excl_off, int32_t* ids_host, float* scores_host) {
    CHECK_ARG(ses && slots && ids_host, "null argument");
    sbr_handle* h = ses->h;
    const Layout& y = h->lay;
    const SesPool& p = ses->p;
    int rc;
    if ((rc = sessions_state_check(ses, "sbr_sessions_rank_candidates")) != SBR_OK) return rc;
    CHECK_ARG(n >= 1 && n <= 0x7fffffff, "sbr_sessions_rank_candidates: n=%lld sessions: at least one", (long long)n);
    CHECK_ARG(k >= 1 && k <= y.N, "k=%d outside [1,N=%d]", k, y.N);
    CHECK_ARG(exclude_mode >= SBR_SESSION_EXCL_NONE && exclude_mode <= SBR_SESSION_EXCL_HISTORY, "unknown exclusion mode %d", exclude_mode);
    if ((rc = sessions_check_slots(ses, "sbr_sessions_rank_candidates", slots, n, false)) != SBR_OK) return rc;
    const int B = y.B;
    CandLists c;
    ExclLists x;
    if ((rc = cand_check(cand_ids, cand_off, n, B, shared, y.N, c)) != SBR_OK) return rc;
    if ((rc = excl_check(excl_ids, excl_off, (int)n, y.N, x)) != SBR_OK) return rc;
    const size_t nk = (size_t)n * k;
    Carver cv;
    const size_t o_slots = cv.take((size_t)n * sizeof(int));
    excl_carve(cv, x);
    cand_carve(cv, c);
    const size_t o_states = cv.take((size_t)B * y.HLt * sizeof(float));
    const CandWork cw = carve_cand_work(cv, c, k);
    const size_t o_oid = cv.take(nk * sizeof(int)), o_osc = cv.take(nk * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    if ((rc = flush_lazy(h, 1)) != SBR_OK) return rc;      // all of W_out^T / b_out current, as sbr_sessions_rank leaves it
    // (pageable host memory: the copy has left the caller's array when it returns)
    SBR_HIP(hipMemcpyAsync(S + o_slots, slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if ((rc = excl_upload(h, S, x)) != SBR_OK || (rc = cand_upload(h, S, c)) != SBR_OK) return rc;
    const int* dslots = (const int*)(S + o_slots);
    float* states = (float*)(S + o_states);
    float* lg = h->A(y.a_logits);
    const bool restricted = cand_rank_restricted(h);
    for (int64_t c0 = 0; c0 < n; c0 += B) {
        const int rows = (int)std::min<int64_t>(B, n - c0);
        SBR_LAUNCH(launch_ses_gather_top(s, p, dslots + c0, rows, states));
        if (!restricted && (rc = project_rows(h, states, rows, lg, 0)) != SBR_OK) return rc;
        ExclSources src;
        if (x.off) src.lists(x.dev_ids(S), x.dev_off(S) + c0);
        src.sessions(dslots + c0, p.ring, p.events, p.ring_len, p.history, exclude_mode);
        if ((rc = cand_rank_chunk(h, S, c, cw, states, lg, c0, rows, src, k, restricted, (int*)(S + o_oid) + (size_t)c0 * k,
                                  (float*)(S + o_osc) + (size_t)c0 * k)) != SBR_OK) return rc;
    }
    SBR_HIP(hipMemcpyAsync(ids_host, S + o_oid, nk * sizeof(int), hipMemcpyDeviceToHost, s));
    if (scores_host) SBR_HIP(hipMemcpyAsync(scores_host, S + o_osc, nk * sizeof(float), hipMemcpyDeviceToHost, s));
    return check_fault(h);
}

// what sbr_evaluate and sbr_cluster_evaluate check about the users, k and the dataset against the engine; on SBR_OK v holds the sorted goals
static int eval_check_args(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int k, SbrEvalView& v) {
    const Layout& y = h->lay;
    int rc;
    if ((rc = sbr_dataset_eval_view(d, &v, 0)) != SBR_OK) return rc;
    CHECK_ARG(n >= 1, "n=%lld users: at least one", (long long)n);
    CHECK_ARG(k >= 1 && k <= y.N, "k=%d outside [1,N=%d]", k, y.N);
    CHECK_ARG(y.F == 1 || (y.F == 2 && v.rate && y.cfg.input_size == y.N + 10),
              "a model with two indices per step needs the ratings attached to the dataset (sbr_dataset_set_options)");
    CHECK_ARG(v.n_items == y.N && (y.cfg.input_size == y.N || y.F == 2), "dataset has %d items, the model %d", v.n_items, y.N);
    CHECK_ARG(v.stream == h->stream, "dataset and engine must share one stream");
    for (int64_t j = 0; j < n; ++j) {
        CHECK_ARG(users[j] >= 0 && users[j] < v.n_users, "users[%lld] = %d outside [0,%lld)", (long long)j, users[j], (long long)v.n_users);
        CHECK_ARG(v.h_off[users[j] + 1] - v.h_off[users[j]] >= 2, "user %d has fewer than two items: nothing to view or no goal", users[j]);
    }
    return sbr_dataset_eval_view(d, &v, 1);      // (first call for this dataset: sorts and uploads the goals)
}

// a chunk's rows become the current batch, in set 0, as sbr_set_batch would leave it; prefix: the rows hold the start of every user's
// sequence (UserPrefix, sbr_evaluate_positions) where they otherwise hold the window of its viewed half (UserSplit)
static int eval_pack_chunk(sbr_handle* h, const SbrEvalView& v, const int* dusers, int rows, bool prefix = false) {
    const Layout& y = h->lay;
    hipStream_t s = h->stream;
    h->bX = (const int*)h->A(y.a_X); h->blen = (const int*)h->A(y.a_len); h->btgt = (const int*)h->A(y.a_tgt);
    h->bsmp = (const int*)h->A(y.a_smp); h->bpop = h->A(y.a_pop);
    h->bb_set = 0; h->bb_unread = false;
    if (rows < y.Bp && SBR_LOSS_IS_MARGIN(y.cfg.loss)) SBR_HIP(hipMemsetAsync(h->A(y.a_tgt), 0xFF, (size_t)y.Bp * y.NT * sizeof(int), s));   // no positives
    SBR_LAUNCH((prefix ? launch_ev_pack_prefix : launch_ev_pack)(s, v, dusers, rows, y.Bp, y.T, y.F, (int*)h->A(y.a_X), (int*)h->A(y.a_len), h->A(y.a_pop)));
    h->n_rows = rows; h->have_batch = true; h->fwd_done = false;
    return SBR_OK;
}

// where an evaluation's exclusion lands in the whole-catalogue scores: WINDOW_ZERO scores the items fed 0.0 and keeps them rankable
static ExclCatalogue eval_sink(float* scores, int N, int exclude_mode) {
    return ExclCatalogue{scores, N, exclude_mode == SBR_EVAL_EXCL_WINDOW_ZERO ? 0.0f : -INFINITY};
}

// The chunk loop of the whole-catalogue evaluations: local_batch users at a time are packed, scored (the very floats sbr_rank ranks;
// lazily stepped rows are flushed) and excluded from the dataset's CSR, then `ranked(c0, rows, scores)` enqueues what the call makes of
// the chunk's score rows.  Everything on the main stream, no host wait.
template <class Ranked>
static int eval_chunks(sbr_handle* h, const SbrEvalView& v, const int* dusers, int64_t n, int exclude_mode, Ranked&& ranked) {
    const Layout& y = h->lay;
    int rc;
    for (int64_t c0 = 0; c0 < n; c0 += y.B) {
        const int rows = (int)std::min<int64_t>(y.B, n - c0);
        if ((rc = eval_pack_chunk(h, v, dusers + c0, rows)) != SBR_OK) return rc;
        if ((rc = full_scores(h, 0)) != SBR_OK) return rc;
        float* lg = h->A(y.a_logits);
        SBR_LAUNCH(launch_exclude(h->stream, rows, ExclSources().dataset(v, dusers + c0, y.T, exclude_mode), eval_sink(lg, y.N, exclude_mode)));
        if ((rc = ranked(c0, rows, lg)) != SBR_OK) return rc;
    }
    return SBR_OK;
}

// One ranking's per-user records of an evaluation call (an sbr_eval_out's device side): sized for all n users of the call, every chunk
// writes at its offset; `oid` holds the ids of every user only when the caller fetches them, otherwise one chunk's
struct EvalRecords {
    const sbr_eval_out* o; int64_t n; int k, words, N;
    size_t npred, hits, first, mask, ihits, oid;
    int* ids_at(char* S, int64_t c0) const { return (int*)(S + oid) + (o->ids ? (size_t)c0 * k : 0); }
};
static bool eval_out_ok(const sbr_eval_out* o) { return o->n_pred && o->hits && o->first_hit; }
static EvalRecords carve_records(Carver& cv, const sbr_eval_out* o, int64_t n, int k, int N, int B) {
    EvalRecords r{o, n, k, (k + 31) / 32, N, 0, 0, 0, 0, 0, 0};
    if (!o) return r;
    r.npred = cv.take((size_t)n * sizeof(int)); r.hits = cv.take((size_t)n * sizeof(int)); r.first = cv.take((size_t)n * sizeof(int));
    r.mask = cv.take(o->hitmask ? (size_t)n * r.words * sizeof(unsigned) : 0); r.ihits = cv.take(o->item_hits ? (size_t)N * sizeof(int) : 0);
    r.oid = cv.take((o->ids ? (size_t)n * k : (size_t)B * k) * sizeof(int));
    return r;
}
// before the chunk loop: item_hits is the one record the chunks add to
static int clear_records(sbr_handle* h, char* S, const EvalRecords& r) {
    if (r.o && r.o->item_hits) SBR_HIP(hipMemsetAsync(S + r.ihits, 0, (size_t)r.N * sizeof(int), h->stream));
    return SBR_OK;
}
// the records of the chunk's users [c0, c0 + rows) from their ranked ids
static int launch_hits(sbr_handle* h, char* S, const EvalRecords& r, const SbrEvalView& v, const int* users, int64_t c0, int rows, const int* ids) {
    SBR_LAUNCH(launch_ev_hits(h->stream, v, users + c0, rows, r.k, ids, (int*)(S + r.npred) + c0, (int*)(S + r.hits) + c0, (int*)(S + r.first) + c0,
                              r.o->hitmask ? (unsigned*)(S + r.mask) + (size_t)c0 * r.words : nullptr, r.o->item_hits ? (int*)(S + r.ihits) : nullptr));
    return SBR_OK;
}
static int fetch_records(sbr_handle* h, const char* S, const EvalRecords& r) {
    const sbr_eval_out* o = r.o;
    hipStream_t s = h->stream;
    const size_t n = (size_t)r.n;
    if (o->ids) SBR_HIP(hipMemcpyAsync(o->ids, S + r.oid, n * r.k * sizeof(int), hipMemcpyDeviceToHost, s));
    SBR_HIP(hipMemcpyAsync(o->n_pred, S + r.npred, n * sizeof(int), hipMemcpyDeviceToHost, s));
    SBR_HIP(hipMemcpyAsync(o->hits, S + r.hits, n * sizeof(int), hipMemcpyDeviceToHost, s));
    SBR_HIP(hipMemcpyAsync(o->first_hit, S + r.first, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (o->hitmask) SBR_HIP(hipMemcpyAsync(o->hitmask, S + r.mask, n * r.words * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (o->item_hits) SBR_HIP(hipMemcpyAsync(o->item_hits, S + r.ihits, (size_t)r.N * sizeof(int), hipMemcpyDeviceToHost, s));
    return SBR_OK;
}

// Whole users evaluated on the device (include/sbr_rnn.h: sbr_evaluate; kernels: sbr_eval.hip).  Per chunk of local_batch users:
// pack -> forward + projection (full_scores) -> exclusion from the dataset's CSR -> sbr_rank's select and sort -> hits, all on the
// main stream; the per-user results of every chunk land at the chunk's offset of arrays sized for the whole call, and the host
// waits once, in check_fault.  The pack writes batch set 0 on the main stream like sbr_set_batch's device-to-device copies, behind every
// reader of the set (sbr_build_batch's comment, sbr_batch.hip), and leaves the handle as that call does.
extern "C" int sbr_evaluate(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int k, int exclude_mode, int32_t* ids_host,
                            int32_t* n_pred_host, int32_t* hits_host, int32_t* first_hit_host, uint32_t* hitmask_host, int32_t* item_hits_host) {
    CHECK_ARG(h && d && users && n_pred_host && hits_host && first_hit_host, "null argument");
    CHECK_ARG(exclude_mode >= SBR_EVAL_EXCL_NONE && exclude_mode <= SBR_EVAL_EXCL_WINDOW_ZERO, "unknown exclusion mode %d", exclude_mode);
    const Layout& y = h->lay;
    SbrEvalView v;
    int rc;
    if ((rc = eval_check_args(h, d, users, n, k, v)) != SBR_OK) return rc;
    const sbr_eval_out out{ids_host, n_pred_host, hits_host, first_hit_host, hitmask_host, item_hits_host};
    const int B = y.B;
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int));
    const EvalRecords rec = carve_records(cv, &out, n, k, y.N, B);
    const RankWork w = carve_rank_work(cv, B, k, k > kRankSortLds);
    const size_t o_osc = cv.take((size_t)B * k * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    // (pageable host memory: the copy has left the caller's array when it returns)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if ((rc = clear_records(h, S, rec)) != SBR_OK) return rc;
    rc = eval_chunks(h, v, dusers, n, exclude_mode, [&](int64_t c0, int rows, float* lg) -> int {
        int* oid = rec.ids_at(S, c0);
        int rc2;
        if ((rc2 = rank_rows(h, S, w, lg, rows, y.N, k, oid, (float*)(S + o_osc))) != SBR_OK) return rc2;
        return launch_hits(h, S, rec, v, dusers, c0, rows, oid);
    });
    if (rc != SBR_OK) return rc;
    if ((rc = fetch_records(h, S, rec)) != SBR_OK) return rc;
    return check_fault(h);          // a forward that gave up must not hand out rankings; the call's one wait for the device
}

// Lazily stepped rows are brought up to date where a call reads them, and WHERE a replay of missed steps is split changes float32
// roundings (sbr_sparse.hip): a training run with such a call in its middle would differ in the last bit from one without.  So once
// steps have been applied, sbr_evaluate_ranks and sbr_evaluate_positions keep the parameters, the optimizer state and the rows'
// last-step words in the ranking scratch and put them back behind the last chunk.
struct LazyKeep {
    bool keep = false;
    size_t np_bytes = 0, o_kp = 0, o_ks = 0, o_kl[2] = {0, 0};
    void carve(Carver& cv, const sbr_handle* h) {
        const Layout& y = h->lay;
        keep = sparse_lazy(h) && h->step_count > 0;
        np_bytes = y.n_params * sizeof(float);
        o_kp = cv.take(keep ? np_bytes : 0); o_ks = cv.take(keep ? y.n_state_arrays * np_bytes : 0);
        for (int b = 0; b < y.n_sparse; ++b) o_kl[b] = cv.take(keep ? (size_t)y.sparse[b].n_rows * sizeof(int) : 0);
    }
    int save(sbr_handle* h, char* S) const {
        if (!keep) return SBR_OK;
        const Layout& y = h->lay;
        hipStream_t s = h->stream;
        SBR_HIP(hipMemcpyAsync(S + o_kp, h->P(0), np_bytes, hipMemcpyDeviceToDevice, s));
        SBR_HIP(hipMemcpyAsync(S + o_ks, h->St(0, 0), y.n_state_arrays * np_bytes, hipMemcpyDeviceToDevice, s));
        for (int b = 0; b < y.n_sparse; ++b)
            SBR_HIP(hipMemcpyAsync(S + o_kl[b], h->A(y.sparse[b].a_last), (size_t)y.sparse[b].n_rows * sizeof(int), hipMemcpyDeviceToDevice, s));
        return SBR_OK;
    }
    int restore(sbr_handle* h, char* S) const {
        if (!keep) return SBR_OK;
        const Layout& y = h->lay;
        hipStream_t s = h->stream;
        SBR_HIP(hipMemcpyAsync(h->P(0), S + o_kp, np_bytes, hipMemcpyDeviceToDevice, s));
        SBR_HIP(hipMemcpyAsync(h->St(0, 0), S + o_ks, y.n_state_arrays * np_bytes, hipMemcpyDeviceToDevice, s));
        for (int b = 0; b < y.n_sparse; ++b)
            SBR_HIP(hipMemcpyAsync(h->A(y.sparse[b].a_last), S + o_kl[b], (size_t)y.sparse[b].n_rows * sizeof(int), hipMemcpyDeviceToDevice, s));
        return SBR_OK;
    }
};

// The place of every goal item in the complete ranking of its user (include/sbr_rnn.h: sbr_evaluate_ranks): sbr_evaluate's chunks with
// one counting kernel (ev_goal_rank_kernel, sbr_eval.hip) where that call selects, sorts and compares.  The offsets of the users' goal
// places follow from the lengths alone: they are written for the caller, and uploaded, before anything is launched.
extern "C" int sbr_evaluate_ranks(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int exclude_mode, int64_t* goal_off_host,
                                  int32_t* ranks_host, int64_t cap, int32_t* n_rankable_host) {
    CHECK_ARG(h && d && users && goal_off_host && ranks_host && n_rankable_host, "null argument");
    CHECK_ARG(exclude_mode >= SBR_EVAL_EXCL_NONE && exclude_mode <= SBR_EVAL_EXCL_WINDOW_ZERO, "unknown exclusion mode %d", exclude_mode);
    const Layout& y = h->lay;
    SbrEvalView v;
    int rc;
    if ((rc = eval_check_args(h, d, users, n, 1, v)) != SBR_OK) return rc;      // (no k here: 1 is inside every catalogue)
    int64_t total = 0;
    auto goal_len = [&](int64_t j) -> int64_t { return UserSplit(v.h_off[users[j]], v.h_off[users[j] + 1], y.T).goal_len(); };
    for (int64_t j = 0; j < n; ++j) total += goal_len(j);
    CHECK_ARG(cap >= total, "cap=%lld: the goals of these users hold %lld items", (long long)cap, (long long)total);
    goal_off_host[0] = 0;
    for (int64_t j = 0; j < n; ++j) goal_off_host[j + 1] = goal_off_host[j] + goal_len(j);
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int)), o_goff = cv.take((size_t)(n + 1) * sizeof(long long));
    const size_t o_ranks = cv.take((size_t)total * sizeof(int)), o_nrk = cv.take((size_t)n * sizeof(int));
    LazyKeep kept;      // training goes on as if the call had not been made
    kept.carve(cv, h);
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    const long long* dgoff = (const long long*)(S + o_goff);
    static_assert(sizeof(long long) == sizeof(int64_t), "the offsets are uploaded as they are");
    // (pageable host memory: the copies have left the caller's arrays when they return)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    SBR_HIP(hipMemcpyAsync(S + o_goff, goal_off_host, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    { const int rck = kept.save(h, S); if (rck != SBR_OK) return rck; }
    rc = eval_chunks(h, v, dusers, n, exclude_mode, [&](int64_t c0, int rows, float* lg) -> int {
        SBR_LAUNCH(launch_ev_goal_rank(s, v, dusers + c0, dgoff + c0, rows, y.N, lg, (int*)(S + o_ranks), (int*)(S + o_nrk) + c0, &h->last_goal_rank_form));
        return SBR_OK;
    });
    { const int rck = kept.restore(h, S); if (rck != SBR_OK) return rck; }      // (also behind a chunk that failed: the call leaves the bits it found)
    if (rc != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(ranks_host, S + o_ranks, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    SBR_HIP(hipMemcpyAsync(n_rankable_host, S + o_nrk, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    return check_fault(h);          // a forward that gave up must not hand out ranks; the call's one wait for the device
}

// The place of the NEXT item at every position of every user's sequence (include/sbr_rnn.h: sbr_evaluate_positions; UserPrefix,
// sbr_common.h).  Per chunk of local_batch users: pack the start of every sequence -> ONE forward pass -> the
// first-occurrence flags of the rows -> per group of up to `slots` positions p = min_history .. the chunk's longest row: the projection
// of those slots of the top layer's states (project_rows: full_scores' launch pair, same mode) and one counting launch
// (ev_next_rank_kernel), which only reads the scores.  Everything on the main stream; the call waits once, in check_fault.  The
// offsets of the users' positions follow from the lengths alone: they are written for the caller, and uploaded, before anything is
// launched.
extern "C" int sbr_evaluate_positions(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int min_history, int exclude_mode,
                                      int64_t* pos_off_host, int32_t* ranks_host, int32_t* n_rankable_host, int64_t cap) {
    CHECK_ARG(h && d && users && pos_off_host && ranks_host && n_rankable_host, "null argument");
    CHECK_ARG(exclude_mode == SBR_EVAL_EXCL_NONE || exclude_mode == SBR_EVAL_EXCL_PREFIX,
              "sbr_evaluate_positions takes SBR_EVAL_EXCL_NONE or SBR_EVAL_EXCL_PREFIX, not mode %d", exclude_mode);
    CHECK_ARG(min_history >= 1, "min_history=%d: a position needs at least one item in front of it", min_history);
    const Layout& y = h->lay;
    // a backwards layer's state at place p has read the items behind p: its slots are no states "after p items"
    CHECK_ARG(y.D == 1, "sbr_evaluate_positions: a bidirectional engine has no state that has seen only the first p items");
    SbrEvalView v;
    int rc;
    if ((rc = eval_check_args(h, d, users, n, 1, v)) != SBR_OK) return rc;      // (no k here: 1 is inside every catalogue)
    auto prefix = [&](int64_t j) { return UserPrefix(v.h_off[users[j]], v.h_off[users[j] + 1], y.T, min_history); };
    int64_t total = 0;
    for (int64_t j = 0; j < n; ++j) total += prefix(j).n_pos();
    CHECK_ARG(cap >= total, "cap=%lld: these users hold %lld positions", (long long)cap, (long long)total);
    pos_off_host[0] = 0;
    for (int64_t j = 0; j < n; ++j) pos_off_host[j + 1] = pos_off_host[j] + prefix(j).n_pos();
    const int B = y.B;
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int)), o_poff = cv.take((size_t)(n + 1) * sizeof(long long));
    const size_t o_ranks = cv.take((size_t)total * sizeof(int)), o_nrk = cv.take((size_t)total * sizeof(int));
    const size_t o_first = cv.take((size_t)B * y.T * sizeof(int));
    // Consecutive slots of a_hs are consecutive rows of ONE matrix: up to kNextRankSlots positions share a projection launch where
    // their scores fit kNextRankScoreBytes of scratch, and where the GEMM's accumulation order does not depend on the rows it carries:
    // the exact-f32 kernel without a workspace (no split-K) and the triage kernel; the one-pass bf16 kernel chooses its tile by the
    // row count, so it keeps one slot per launch, in a_logits, with full_scores' n_rows.
    const size_t slot_floats = (size_t)y.Bp * y.N;
    const int slots = scores_gemm_mode(h).one_pass ? 1 : (int)std::max<size_t>(1, std::min<size_t>(kNextRankSlots, kNextRankScoreBytes / (slot_floats * sizeof(float))));
    const size_t o_scores = cv.take(slots > 1 ? slots * slot_floats * sizeof(float) : 0);
    LazyKeep kept;      // training goes on as if the call had not been made
    kept.carve(cv, h);
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    const long long* dpoff = (const long long*)(S + o_poff);
    int* first = (int*)(S + o_first);
    float* scores = slots > 1 ? (float*)(S + o_scores) : h->A(y.a_logits);
    h->last_next_rank_slots = slots;
    // (pageable host memory: the copies have left the caller's arrays when they return)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    SBR_HIP(hipMemcpyAsync(S + o_poff, pos_off_host, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    { const int rck = kept.save(h, S); if (rck != SBR_OK) return rck; }
    const LayerLayout& top = y.layer[y.L - 1];
    auto chunks = [&]() -> int {
        for (int64_t c0 = 0; c0 < n; c0 += B) {
            const int rows = (int)std::min<int64_t>(B, n - c0);
            int last = 0;                                              // the chunk's longest row
            for (int r = 0; r < rows; ++r) last = std::max(last, prefix(c0 + r).last_pos());
            int rc2;
            // the chunk becomes the current batch (eval_pack_chunk with the prefix policy)
            if ((rc2 = eval_pack_chunk(h, v, dusers + c0, rows, true)) != SBR_OK) return rc2;
            if ((rc2 = forward_current(h)) != SBR_OK) return rc2;
            if (exclude_mode == SBR_EVAL_EXCL_PREFIX) SBR_LAUNCH(launch_ev_first_seen(s, h->bX, h->blen, rows, y.T, y.F, first));
            for (int p0 = min_history; p0 <= last; p0 += slots) {
                const int k = std::min(slots, last - p0 + 1);
                // slot p = the state after p items: for a row of exactly p items, the very floats of h_last.  k slots = the rows
                // [p0 * Bp, (p0 + k - 1) * Bp + rows) of a_hs (the padded rows between two slots are projected along)
                if ((rc2 = project_rows(h, h->A(top.a_hs) + (size_t)p0 * y.Bp * top.Hp, (k - 1) * y.Bp + rows, scores, 0)) != SBR_OK) return rc2;
                SBR_LAUNCH(launch_ev_next_rank(s, v, dusers + c0, dpoff + c0, h->bX, h->blen, first, rows, y.T, y.F, y.N, p0, k, min_history,
                                               exclude_mode == SBR_EVAL_EXCL_PREFIX, scores, slot_floats, (int*)(S + o_ranks), (int*)(S + o_nrk),
                                               &h->last_next_rank_form));
            }
        }
        return SBR_OK;
    };
    rc = chunks();
    { const int rck = kept.restore(h, S); if (rck != SBR_OK) return rck; }      // (also behind a chunk that failed: the call leaves the bits it found)
    if (rc != SBR_OK) return rc;
    if (total) {
        SBR_HIP(hipMemcpyAsync(ranks_host, S + o_ranks, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
        SBR_HIP(hipMemcpyAsync(n_rankable_host, S + o_nrk, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    return check_fault(h);          // a forward that gave up must not hand out ranks; the call's one wait for the device
}

// what both log-probability calls refuse about the engine's state before anything else
static int logprob_state_check(const sbr_handle* h, const char* call) {
    if (h->st.step_open || h->st.train_fwd_open) { sbr_set_error("%s: a training step is open (finish it with sbr_apply_update)", call); return SBR_ESTATE; }
    if (h->lag_pending >= 0) { sbr_set_error("%s: a lagged cost is pending (collect it with sbr_lagged_flush)", call); return SBR_ESTATE; }
    return SBR_OK;
}

// The log-probability of every goal item under the softmax over its row's rankable items (include/sbr_rnn.h: sbr_evaluate_logprob;
// DESIGN.md 3u): sbr_evaluate_ranks' call -- the same split, window, chunks, exclusion launch, offsets and keep-and-restore -- with the
// float reduction (ev_goal_logprob_kernel, sbr_eval.hip) behind the exclusion, and ev_goal_rank_kernel in front of it on the same row
// when the caller takes ranks or n_rankable.
extern "C" int sbr_evaluate_logprob(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int exclude_mode, int64_t* goal_off_host,
                                    float* logp_host, int64_t cap, float* log_z_host, int32_t* ranks_host, int32_t* n_rankable_host) {
    CHECK_ARG(h && d && users && goal_off_host && logp_host, "null argument");
    CHECK_ARG(exclude_mode >= SBR_EVAL_EXCL_NONE && exclude_mode <= SBR_EVAL_EXCL_WINDOW,
              "sbr_evaluate_logprob takes SBR_EVAL_EXCL_NONE, _VIEWED or _WINDOW, not mode %d (an item scored 0.0 is no exclusion from a softmax)", exclude_mode);
    const Layout& y = h->lay;
    SbrEvalView v;
    int rc;
    if ((rc = logprob_state_check(h, "sbr_evaluate_logprob")) != SBR_OK) return rc;
    if ((rc = eval_check_args(h, d, users, n, 1, v)) != SBR_OK) return rc;      // (no k here: 1 is inside every catalogue)
    int64_t total = 0;
    auto goal_len = [&](int64_t j) -> int64_t { return UserSplit(v.h_off[users[j]], v.h_off[users[j] + 1], y.T).goal_len(); };
    for (int64_t j = 0; j < n; ++j) total += goal_len(j);
    CHECK_ARG(cap >= total, "cap=%lld: the goals of these users hold %lld items", (long long)cap, (long long)total);
    goal_off_host[0] = 0;
    for (int64_t j = 0; j < n; ++j) goal_off_host[j + 1] = goal_off_host[j] + goal_len(j);
    const bool counts = ranks_host || n_rankable_host;
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int)), o_goff = cv.take((size_t)(n + 1) * sizeof(long long));
    const size_t o_logp = cv.take((size_t)total * sizeof(float)), o_logz = cv.take((size_t)n * sizeof(float));
    const size_t o_ranks = cv.take(counts ? (size_t)total * sizeof(int) : 0), o_nrk = cv.take(counts ? (size_t)n * sizeof(int) : 0);
    LazyKeep kept;      // training goes on as if the call had not been made
    kept.carve(cv, h);
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    const long long* dgoff = (const long long*)(S + o_goff);
    // (pageable host memory: the copies have left the caller's arrays when they return)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    SBR_HIP(hipMemcpyAsync(S + o_goff, goal_off_host, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    { const int rck = kept.save(h, S); if (rck != SBR_OK) return rck; }
    rc = eval_chunks(h, v, dusers, n, exclude_mode, [&](int64_t c0, int rows, float* lg) -> int {
        if (counts)
            SBR_LAUNCH(launch_ev_goal_rank(s, v, dusers + c0, dgoff + c0, rows, y.N, lg, (int*)(S + o_ranks), (int*)(S + o_nrk) + c0, &h->last_goal_rank_form));
        SBR_LAUNCH(launch_ev_goal_logprob(s, v, dusers + c0, dgoff + c0, rows, y.N, lg, (float*)(S + o_logp), (float*)(S + o_logz) + c0,
                                          &h->last_logprob_form));
        return SBR_OK;
    });
    { const int rck = kept.restore(h, S); if (rck != SBR_OK) return rck; }      // (also behind a chunk that failed: the call leaves the bits it found)
    if (rc != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(logp_host, S + o_logp, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s));
    if (log_z_host) SBR_HIP(hipMemcpyAsync(log_z_host, S + o_logz, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (ranks_host) SBR_HIP(hipMemcpyAsync(ranks_host, S + o_ranks, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    if (n_rankable_host) SBR_HIP(hipMemcpyAsync(n_rankable_host, S + o_nrk, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    return check_fault(h);          // a forward that gave up must not hand out results; the call's one wait for the device
}

// The log-probability of the NEXT item at every position (include/sbr_rnn.h: sbr_evaluate_positions_logprob): sbr_evaluate_positions'
// call -- the same prefix, chunks, groups of slots and projections -- with, per group, the integer counts first (only when the caller
// takes ranks or n_rankable: they read the scores as projected) and then ev_next_logprob_kernel, which writes -inf at the prefix's ids
// into its own (row, slot) score rows before it reduces them.  The scores of a group are projected anew for the next one.
extern "C" int sbr_evaluate_positions_logprob(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int min_history, int exclude_mode,
                                              int64_t* pos_off_host, float* logp_host, float* log_z_host, int32_t* ranks_host,
                                              int32_t* n_rankable_host, int64_t cap) {
    CHECK_ARG(h && d && users && pos_off_host && logp_host, "null argument");
    CHECK_ARG(exclude_mode == SBR_EVAL_EXCL_NONE || exclude_mode == SBR_EVAL_EXCL_PREFIX,
              "sbr_evaluate_positions_logprob takes SBR_EVAL_EXCL_NONE or SBR_EVAL_EXCL_PREFIX, not mode %d", exclude_mode);
    CHECK_ARG(min_history >= 1, "min_history=%d: a position needs at least one item in front of it", min_history);
    const Layout& y = h->lay;
    // a backwards layer's state at place p has read the items behind p: its slots are no states "after p items"
    CHECK_ARG(y.D == 1, "sbr_evaluate_positions_logprob: a bidirectional engine has no state that has seen only the first p items");
    SbrEvalView v;
    int rc;
    if ((rc = logprob_state_check(h, "sbr_evaluate_positions_logprob")) != SBR_OK) return rc;
    if ((rc = eval_check_args(h, d, users, n, 1, v)) != SBR_OK) return rc;      // (no k here: 1 is inside every catalogue)
    auto prefix = [&](int64_t j) { return UserPrefix(v.h_off[users[j]], v.h_off[users[j] + 1], y.T, min_history); };
    int64_t total = 0;
    for (int64_t j = 0; j < n; ++j) total += prefix(j).n_pos();
    CHECK_ARG(cap >= total, "cap=%lld: these users hold %lld positions", (long long)cap, (long long)total);
    pos_off_host[0] = 0;
    for (int64_t j = 0; j < n; ++j) pos_off_host[j + 1] = pos_off_host[j] + prefix(j).n_pos();
    const int B = y.B;
    const bool counts = ranks_host || n_rankable_host, excl = exclude_mode == SBR_EVAL_EXCL_PREFIX;
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int)), o_poff = cv.take((size_t)(n + 1) * sizeof(long long));
    const size_t o_logp = cv.take((size_t)total * sizeof(float)), o_logz = cv.take(log_z_host ? (size_t)total * sizeof(float) : 0);
    const size_t o_ranks = cv.take(counts ? (size_t)total * sizeof(int) : 0), o_nrk = cv.take(counts ? (size_t)total * sizeof(int) : 0);
    const size_t o_first = cv.take((size_t)B * y.T * sizeof(int));
    // the slots of a group: sbr_evaluate_positions' rule, so that a position's scores are the floats that call counts
    const size_t slot_floats = (size_t)y.Bp * y.N;
    const int slots = scores_gemm_mode(h).one_pass ? 1 : (int)std::max<size_t>(1, std::min<size_t>(kNextRankSlots, kNextRankScoreBytes / (slot_floats * sizeof(float))));
    const size_t o_scores = cv.take(slots > 1 ? slots * slot_floats * sizeof(float) : 0);
    LazyKeep kept;      // training goes on as if the call had not been made
    kept.carve(cv, h);
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    const long long* dpoff = (const long long*)(S + o_poff);
    int* first = (int*)(S + o_first);
    float* scores = slots > 1 ? (float*)(S + o_scores) : h->A(y.a_logits);
    float* dlogz = log_z_host ? (float*)(S + o_logz) : nullptr;
    h->last_next_rank_slots = slots;
    // (pageable host memory: the copies have left the caller's arrays when they return)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    SBR_HIP(hipMemcpyAsync(S + o_poff, pos_off_host, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    { const int rck = kept.save(h, S); if (rck != SBR_OK) return rck; }
    const LayerLayout& top = y.layer[y.L - 1];
    auto chunks = [&]() -> int {
        for (int64_t c0 = 0; c0 < n; c0 += B) {
            const int rows = (int)std::min<int64_t>(B, n - c0);
            int last = 0;                                              // the chunk's longest row
            for (int r = 0; r < rows; ++r) last = std::max(last, prefix(c0 + r).last_pos());
            int rc2;
            if ((rc2 = eval_pack_chunk(h, v, dusers + c0, rows, true)) != SBR_OK) return rc2;
            if ((rc2 = forward_current(h)) != SBR_OK) return rc2;
            if (excl && counts) SBR_LAUNCH(launch_ev_first_seen(s, h->bX, h->blen, rows, y.T, y.F, first));
            for (int p0 = min_history; p0 <= last; p0 += slots) {
                const int k = std::min(slots, last - p0 + 1);
                if ((rc2 = project_rows(h, h->A(top.a_hs) + (size_t)p0 * y.Bp * top.Hp, (k - 1) * y.Bp + rows, scores, 0)) != SBR_OK) return rc2;
                if (counts)
                    SBR_LAUNCH(launch_ev_next_rank(s, v, dusers + c0, dpoff + c0, h->bX, h->blen, first, rows, y.T, y.F, y.N, p0, k, min_history,
                                                   excl, scores, slot_floats, (int*)(S + o_ranks), (int*)(S + o_nrk), &h->last_next_rank_form));
                SBR_LAUNCH(launch_ev_next_logprob(s, v, dusers + c0, dpoff + c0, h->bX, h->blen, rows, y.T, y.F, y.N, p0, k, min_history, excl,
                                                  scores, slot_floats, (float*)(S + o_logp), dlogz, &h->last_logprob_form));
            }
        }
        return SBR_OK;
    };
    rc = chunks();
    { const int rck = kept.restore(h, S); if (rck != SBR_OK) return rck; }      // (also behind a chunk that failed: the call leaves the bits it found)
    if (rc != SBR_OK) return rc;
    if (total) {
        SBR_HIP(hipMemcpyAsync(logp_host, S + o_logp, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s));
        if (log_z_host) SBR_HIP(hipMemcpyAsync(log_z_host, S + o_logz, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s));
        if (ranks_host) SBR_HIP(hipMemcpyAsync(ranks_host, S + o_ranks, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
        if (n_rankable_host) SBR_HIP(hipMemcpyAsync(n_rankable_host, S + o_nrk, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    return check_fault(h);          // a forward that gave up must not hand out results; the call's one wait for the device
}

// The test hook of the float reduction (include/sbr_rnn.h: sbr_debug_row_logprob): row_log_z on the caller's device rows, on the engine's
// stream; the scores are only read.  Waits for the device.
extern "C" int sbr_debug_row_logprob(sbr_handle* h, const float* scores_dev, int64_t ld, int64_t rows, int32_t N, const int32_t* goal_ids_dev,
                                     int32_t goals_per_row, float* logp_dev, float* log_z_dev) {
    CHECK_ARG(h && scores_dev && (logp_dev || goals_per_row == 0) && (goal_ids_dev || goals_per_row == 0), "null argument");
    CHECK_ARG(N >= 1 && ld >= N && rows >= 0 && rows <= 0x7fffffff && goals_per_row >= 0, "N=%d, ld=%lld, rows=%lld, goals_per_row=%d: N >= 1, ld >= N, counts >= 0",
              N, (long long)ld, (long long)rows, goals_per_row);
    SBR_LAUNCH(launch_debug_row_logprob(h->stream, scores_dev, (size_t)ld, (int)rows, N, goal_ids_dev, goals_per_row, logp_dev, log_z_dev,
                                        &h->last_logprob_form));
    SBR_HIP(hipStreamSynchronize(h->stream));
    return SBR_OK;
}

// what sbr_dataset_set_tables asks of sample_cdf
static int neg_cdf_check(const double* cdf, int N) {
    for (int i = 1; i < N; ++i) CHECK_ARG(cdf[i] >= cdf[i - 1], "neg_cdf must be non-decreasing (at item %d)", i);
    CHECK_ARG(cdf[N - 1] > 0, "neg_cdf has no mass");
    return SBR_OK;
}
static int neg_count_check(int n_negatives, int N) {
    CHECK_ARG(n_negatives >= 1 && n_negatives <= std::min(N - 1, SBR_EVAL_MAX_NEGATIVES), "n_negatives=%d outside [1,min(N - 1,%d)=%d]",
              n_negatives, SBR_EVAL_MAX_NEGATIVES, std::min(N - 1, SBR_EVAL_MAX_NEGATIVES));
    return SBR_OK;
}

// The draw of sbr_evaluate_candidates restated on the host, one attempt after the other (the rule: ev_neg_seed, sbr_common.h):
// pure host code, no device, no handle.
extern "C" int sbr_eval_negatives_host(const int32_t* seq, int32_t L, int32_t user, int32_t n_items, int32_t n_negatives, uint64_t seed,
                                       const double* neg_cdf, int32_t* out, int32_t* n_out) {
    CHECK_ARG(out && n_out && L >= 0 && (seq || L == 0), "null argument");
    CHECK_ARG(n_items >= 2 && user >= 0, "n_items=%d, user=%d: at least two items, a user id >= 0", n_items, user);
    int rc;
    if ((rc = neg_count_check(n_negatives, n_items)) != SBR_OK) return rc;
    if (neg_cdf && (rc = neg_cdf_check(neg_cdf, n_items)) != SBR_OK) return rc;
    std::vector<int> sorted(seq, seq + L);
    std::sort(sorted.begin(), sorted.end());
    std::vector<char> taken((size_t)n_items, 0);
    const unsigned long long su = ev_neg_seed(seed, user);
    int na = 0;
    for (int t = 0; t < ev_neg_attempts(n_negatives) && na < n_negatives; ++t) {
        const int it = bb_draw_item(su, t, neg_cdf, n_items);
        if (taken[it] || std::binary_search(sorted.begin(), sorted.end(), it)) continue;
        taken[it] = 1;
        out[na++] = it;
    }
    for (int i = na; i < n_negatives; ++i) out[i] = -1;
    *n_out = na;
    return SBR_OK;
}

// Every goal item ranked among the candidate set of its user (include/sbr_rnn.h: sbr_evaluate_candidates; kernels: sbr_eval_cand.hip;
// DESIGN.md 3q): sbr_evaluate_ranks' chunks -- pack, forward, keep-and-restore of lazily stepped rows -- with, per chunk, the build of
// the merged lists (ev_cand_build_kernel), sbr_rank_candidates' scoring of them (launch_cand_score, or the full projection and
// launch_crk_gather) and one counting kernel over the compact rows (ev_cand_place_kernel).  Where a row's merged list lies follows
// from the lengths alone -- its candidates (or n_negatives) plus its goal places, an upper bound that the kernel pads --, so the offsets
// and the width of every chunk's compact matrix are host values: nothing waits for the device before the end of the call.
extern "C" int sbr_evaluate_candidates(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int exclude_mode,
                                       const int32_t* cand_ids, const int64_t* cand_off, int32_t n_negatives, uint64_t seed,
                                       const double* neg_cdf, int64_t* goal_off_host, int32_t* ranks_host, int64_t cap, int32_t* n_cand_host,
                                       int32_t* negatives_host) {
    CHECK_ARG(h && d && users && goal_off_host && ranks_host && n_cand_host, "null argument");
    if (h->st.step_open || h->st.train_fwd_open) {
        sbr_set_error("sbr_evaluate_candidates: a training step is open (finish it with sbr_apply_update)");
        return SBR_ESTATE;
    }
    CHECK_ARG(exclude_mode != SBR_EVAL_EXCL_WINDOW_ZERO, "sbr_evaluate_candidates: SBR_EVAL_EXCL_WINDOW_ZERO scores the items fed 0.0 in the "
              "whole-catalogue matrix; the compact candidate scores have no such mode (take SBR_EVAL_EXCL_WINDOW or sbr_evaluate_ranks)");
    CHECK_ARG(exclude_mode >= SBR_EVAL_EXCL_NONE && exclude_mode <= SBR_EVAL_EXCL_WINDOW, "unknown exclusion mode %d", exclude_mode);
    const bool expl = cand_ids || cand_off;
    CHECK_ARG(!(expl && n_negatives != 0), "explicit lists (cand_ids / cand_off) and n_negatives=%d: exactly one candidate source", n_negatives);
    CHECK_ARG(expl || n_negatives != 0, "no candidate source: neither cand_ids / cand_off nor n_negatives");
    CHECK_ARG(!expl || !neg_cdf, "neg_cdf belongs to the sampled negatives, not to explicit lists");
    CHECK_ARG(!expl || !negatives_host, "negatives_host belongs to the sampled negatives: explicit lists are the caller's");
    const Layout& y = h->lay;
    SbrEvalView v;
    int rc;
    if ((rc = eval_check_args(h, d, users, n, 1, v)) != SBR_OK) return rc;      // (no k here: 1 is inside every catalogue)
    const int B = y.B, N = y.N;
    CandLists c;
    if (expl) {
        if ((rc = cand_check(cand_ids, cand_off, n, B, 0, N, c)) != SBR_OK) return rc;
    } else {
        if ((rc = neg_count_check(n_negatives, N)) != SBR_OK) return rc;
        if (neg_cdf && (rc = neg_cdf_check(neg_cdf, N)) != SBR_OK) return rc;
    }
    auto goal_len = [&](int64_t j) -> int64_t { return UserSplit(v.h_off[users[j]], v.h_off[users[j] + 1], y.T).goal_len(); };
    // where the merged lists lie: row j holds at most its candidates and one entry per goal place
    std::vector<long long> cap_off((size_t)n + 1, 0);
    int64_t total = 0, chunk_cap = 0;
    int lmax_all = 4;
    for (int64_t c0 = 0; c0 < n; c0 += B) {
        int64_t widest = 0;
        for (int64_t j = c0; j < std::min<int64_t>(n, c0 + B); ++j) {
            const int64_t w = (expl ? cand_off[j + 1] - cand_off[j] : (int64_t)n_negatives) + goal_len(j);
            cap_off[j + 1] = cap_off[j] + w;
            widest = std::max(widest, w);
            total += goal_len(j);
        }
        const int64_t in_chunk = cap_off[std::min<int64_t>(n, c0 + B)] - cap_off[c0];
        CHECK_ARG(in_chunk <= 0x7fffffff && widest <= 0x7ffffff0, "the lists and goals of the %d users from users[%lld] hold %lld ids, at most 2^31 - 1 per chunk",
                  B, (long long)c0, (long long)in_chunk);
        chunk_cap = std::max(chunk_cap, in_chunk);
        lmax_all = std::max(lmax_all, (int)((widest + 3) / 4 * 4));
    }
    CHECK_ARG(cap >= total, "cap=%lld: the goals of these users hold %lld items", (long long)cap, (long long)total);
    goal_off_host[0] = 0;
    for (int64_t j = 0; j < n; ++j) goal_off_host[j + 1] = goal_off_host[j] + goal_len(j);
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int)), o_goff = cv.take((size_t)(n + 1) * sizeof(long long));
    const size_t o_coff = cv.take((size_t)(n + 1) * sizeof(long long));
    const size_t o_ranks = cv.take((size_t)total * sizeof(int)), o_ncand = cv.take((size_t)n * sizeof(int));
    const size_t o_neg = cv.take(negatives_host ? (size_t)n * n_negatives * sizeof(int) : 0);
    const size_t o_cdf = cv.take(neg_cdf ? (size_t)N * sizeof(double) : 0);
    if (expl) cand_carve(cv, c);
    const size_t o_moff = cv.take((size_t)(B + 1) * sizeof(int)), o_csel = cv.take((size_t)B * sizeof(int)), o_mlen = cv.take((size_t)B * sizeof(int));
    const size_t o_mem = cv.take((size_t)chunk_cap * sizeof(int)), o_flag = cv.take((size_t)chunk_cap);
    const size_t o_cs = cv.take((size_t)B * lmax_all * sizeof(float));
    LazyKeep kept;      // training goes on as if the call had not been made
    kept.carve(cv, h);
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    const long long* dgoff = (const long long*)(S + o_goff);
    const long long* dcoff = (const long long*)(S + o_coff);
    // (pageable host memory: the copies have left the host arrays when they return)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    SBR_HIP(hipMemcpyAsync(S + o_goff, goal_off_host, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    SBR_HIP(hipMemcpyAsync(S + o_coff, cap_off.data(), (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    if (neg_cdf) SBR_HIP(hipMemcpyAsync(S + o_cdf, neg_cdf, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
    if (expl && (rc = cand_upload(h, S, c)) != SBR_OK) return rc;      // once per call, as sbr_rank_candidates uploads them
    { const int rck = kept.save(h, S); if (rck != SBR_OK) return rck; }
    const bool restricted = cand_rank_restricted(h);
    int* mem = (int*)(S + o_mem);
    int* moff = (int*)(S + o_moff);
    int* csel = (int*)(S + o_csel);
    int* mlen = (int*)(S + o_mlen);
    unsigned char* flag = (unsigned char*)(S + o_flag);
    float* cs = (float*)(S + o_cs);
    auto chunks = [&]() -> int {
        for (int64_t c0 = 0; c0 < n; c0 += B) {
            const int rows = (int)std::min<int64_t>(B, n - c0);
            int rc2;
            if ((rc2 = eval_pack_chunk(h, v, dusers + c0, rows)) != SBR_OK) return rc2;
            // restricted: the candidates are scored from the hidden state; otherwise the very floats sbr_rank ranks, gathered
            if ((rc2 = restricted ? forward_current(h) : full_scores(h, 0)) != SBR_OK) return rc2;
            long long widest = 0;
            for (int64_t j = c0; j < c0 + rows; ++j) widest = std::max(widest, cap_off[j + 1] - cap_off[j]);
            const int lmax = (int)std::max<long long>(4, (widest + 3) / 4 * 4);      // (rounded up to 4 as the cluster road's)
            EvCandBuild a;
            a.users = dusers + c0; a.rows = rows; a.N = N;
            a.cand_ids = expl ? c.dev_ids(S) : nullptr; a.cand_off = expl ? c.dev_off(S) + c0 : nullptr;
            a.n_neg = expl ? 0 : n_negatives; a.seed = seed; a.cdf = neg_cdf ? (const double*)(S + o_cdf) : nullptr;
            a.hash_slots = expl ? 0 : ev_neg_hash_slots(n_negatives);
            a.negatives = negatives_host ? (int*)(S + o_neg) + (size_t)c0 * n_negatives : nullptr;
            a.cap_off = dcoff + c0;
            a.moff = moff; a.mem = mem; a.flag = flag; a.mlen = mlen; a.csel = csel;
            SBR_LAUNCH(launch_ev_cand_build(s, v, a));
            if (restricted)
                SBR_LAUNCH(launch_cand_score(s, h_last(h), y.HLt, h->P(y.p_WoutT), h->P(y.p_bout), y.HLt, mem, moff, rows, lmax, cs));
            else
                SBR_LAUNCH(launch_crk_gather(s, h->A(y.a_logits), N, csel, mem, moff, rows, lmax, cs));
            h->last_eval_cand_form = restricted ? 1 : 2;
            h->last_eval_cand_lmax = lmax;
            SBR_LAUNCH(launch_ev_cand_place(s, v, dusers + c0, dgoff + c0, rows, y.T, N, exclude_mode, mem, moff, flag, mlen, cs, lmax,
                                            (int*)(S + o_ranks), (int*)(S + o_ncand) + c0));
        }
        return SBR_OK;
    };
    rc = chunks();
    { const int rck = kept.restore(h, S); if (rck != SBR_OK) return rck; }      // (also behind a chunk that failed: the call leaves the bits it found)
    if (rc != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(ranks_host, S + o_ranks, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
    SBR_HIP(hipMemcpyAsync(n_cand_host, S + o_ncand, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (negatives_host) SBR_HIP(hipMemcpyAsync(negatives_host, S + o_neg, (size_t)n * n_negatives * sizeof(int), hipMemcpyDeviceToHost, s));
    return check_fault(h);          // a forward that gave up must not hand out ranks; the call's one wait for the device
}

int cluster_fits_engine(const sbr_cluster* c, const sbr_handle* h) {
    const Layout& y = h->lay;
    const int HL = y.cfg.layers[y.L - 1];
    CHECK_ARG(c->cfg.n_items == y.N, "the cluster head has %d items, the engine %d", c->cfg.n_items, y.N);
    CHECK_ARG(c->cfg.n_hidden == y.D * HL && c->cfg.hidden_split == HL, "the cluster head reads %d features (split %d), the engine's user representation has %d (split %d)",
              c->cfg.n_hidden, c->cfg.hidden_split, y.D * HL, HL);
    CHECK_ARG(c->stream == h->stream, "the cluster head and the engine are on different streams");
    return SBR_OK;
}

// the restricted kernel restates the exact-f32 projection; the bf16 and the triage projections round differently, and their
// scores are gathered from the matrix those kernels write
static bool cluster_rank_restricted(const sbr_handle* h) {
    return h->sw.cluster_rank && !(h->lay.cfg.flags & SBR_FLAG_BF16_PROJECTION) && !simple_gemm(h);
}

// cs [rows][lmax]: the scores of the members of every row's cluster csel[row], restricted (scored from h_last; o_grp: launch_crk_group's
// words in the scratch) or gathered from the full scores
static int cluster_scores(sbr_cluster* c, sbr_handle* h, char* S, size_t o_grp, const int* csel, int rows, int lmax, float* cs, bool restricted) {
    const Layout& y = h->lay;
    const int C = c->cfg.n_clusters;
    if (restricted) {
        SBR_LAUNCH(launch_crk_group(h->stream, csel, rows, C, (int*)(S + o_grp)));
        SBR_LAUNCH(launch_crk_score(h->stream, h_last(h), y.HLt, h->P(y.p_WoutT), h->P(y.p_bout), y.HLt, c->mem_ids, c->mem_off,
                                    (const int*)(S + o_grp), rows, C, lmax, cs));
    } else
        SBR_LAUNCH(launch_crk_gather(h->stream, h->A(y.a_logits), y.N, csel, c->mem_ids, c->mem_off, rows, lmax, cs));
    h->last_cluster_rank_form = restricted ? 1 : 2;
    return SBR_OK;
}

// Ranking inside each row's item cluster (RNNCluster.predict_function for a whole batch, rnn_cluster.py:302-325; kernels and the
// accumulation-order argument: sbr_cluster_rank.hip).  The member lists are the cluster object's, everything a call needs beyond
// them sits in the handle's ranking scratch.
extern "C" int sbr_cluster_rank(sbr_cluster* c, sbr_handle* h, int k, int exclude_input, const int32_t* excl_ids, const int64_t* excl_off,
                                int32_t* ids_host, float* scores_host, int32_t* cluster_host, int32_t* size_host) {
    CHECK_ARG(c && h && ids_host, "null argument");
    if (!h->have_batch) { sbr_set_error("sbr_cluster_rank: no batch set"); return SBR_ESTATE; }
    const Layout& y = h->lay;
    const int rows = h->n_rows, C = c->cfg.n_clusters;
    int rc;
    if ((rc = cluster_fits_engine(c, h)) != SBR_OK) return rc;
    CHECK_ARG(k >= 1 && k <= y.N, "k=%d outside [1,N=%d]", k, y.N);
    ExclLists x;
    if ((rc = excl_check(excl_ids, excl_off, rows, y.N, x)) != SBR_OK) return rc;
    if ((rc = sbr_cluster_build_lists(c)) != SBR_OK) return rc;      // (cached until R changes: sizes and Lmax are host values)
    const int lmax = c->lmax, kk = std::min(k, lmax);
    const size_t rk = (size_t)rows * k, rkk = (size_t)rows * kk;
    Carver cv;
    excl_carve(cv, x);
    const size_t o_csel = cv.take((size_t)rows * sizeof(int)), o_grp = cv.take(sbr_crk_group_words(rows, C) * sizeof(int));
    const size_t o_cs = cv.take((size_t)rows * lmax * sizeof(float));
    const RankWork w = carve_rank_work(cv, rows, kk, kk > kRankSortLds);      // the cluster matrix is ranked to kk places
    const size_t o_pos = cv.take(rkk * sizeof(int)), o_psc = cv.take(rkk * sizeof(float));
    const size_t o_oid = cv.take(rk * sizeof(int)), o_osc = cv.take(rk * sizeof(float)), o_size = cv.take((size_t)rows * sizeof(int));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    int* csel = (int*)(S + o_csel);
    float* cs = (float*)(S + o_cs);
    const bool restricted = cluster_rank_restricted(h);
    if ((rc = restricted ? forward_current(h) : full_scores(h, 0)) != SBR_OK) return rc;
    if ((rc = excl_upload(h, S, x)) != SBR_OK) return rc;
    if ((rc = sbr_cluster_select(c, h_last(h), y.HLt, y.D == 2 ? y.HLp : 0, rows, csel, nullptr)) != SBR_OK) return rc;
    if ((rc = cluster_scores(c, h, S, o_grp, csel, rows, lmax, cs, restricted)) != SBR_OK) return rc;
    SBR_LAUNCH(launch_exclude(h->stream, rows, excl_sources(h, S, x, exclude_input), ExclCluster{cs, lmax, csel, C, c->mem_ids, c->mem_off, y.N}));
    if ((rc = rank_rows(h, S, w, cs, rows, lmax, kk, (int*)(S + o_pos), (float*)(S + o_psc))) != SBR_OK) return rc;
    SBR_LAUNCH(launch_crk_translate(h->stream, (const int*)(S + o_pos), (const float*)(S + o_psc), kk, k, csel, c->mem_ids, c->mem_off, rows,
                                    (int*)(S + o_oid), (float*)(S + o_osc), (int*)(S + o_size)));
    SBR_HIP(hipMemcpyAsync(ids_host, S + o_oid, rk * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (scores_host) SBR_HIP(hipMemcpyAsync(scores_host, S + o_osc, rk * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (cluster_host) SBR_HIP(hipMemcpyAsync(cluster_host, csel, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (size_host) SBR_HIP(hipMemcpyAsync(size_host, S + o_size, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return check_fault(h);          // a forward that gave up must not hand out rankings
}

// Whole users of a cluster model evaluated on the device (include/sbr_rnn.h: sbr_cluster_evaluate; kernels: sbr_cluster_eval.hip and
// the ones sbr_evaluate and sbr_cluster_rank launch).  Per chunk of local_batch users: pack -> forward (+ projection where a full score
// row is read) -> cluster selection -> the cluster ranking's score matrix, taken BEFORE any exclusion touches the full scores ->
// [the whole-catalogue ranking, as sbr_evaluate runs it] -> exclusion, select, sort[, translate], hits of the cluster ranking.  All on
// the main stream; results land at the chunk's offset of arrays sized for the whole call and the host waits once, in check_fault.
extern "C" int sbr_cluster_evaluate(sbr_cluster* c, sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int k, int road,
                                    int exclude_mode, const sbr_eval_out* whole, const sbr_eval_out* inside, int32_t* cluster_host,
                                    int32_t* size_host, int32_t* cluster_use_host) {
    CHECK_ARG(c && h && d && users && inside && cluster_host, "null argument");
    CHECK_ARG(eval_out_ok(inside) && (!whole || eval_out_ok(whole)), "n_pred, hits and first_hit of a given sbr_eval_out are required");
    CHECK_ARG(road == SBR_CEVAL_LISTS || road == SBR_CEVAL_PRODUCT, "unknown road %d", road);
    const bool product = road == SBR_CEVAL_PRODUCT;
    if (product) {
        CHECK_ARG(exclude_mode == SBR_EVAL_EXCL_NONE || exclude_mode == SBR_EVAL_EXCL_WINDOW,
                  "the PRODUCT road takes SBR_EVAL_EXCL_NONE or SBR_EVAL_EXCL_WINDOW, not mode %d", exclude_mode);
        CHECK_ARG(!size_host, "size_host is the LISTS road's: the PRODUCT road ranks the whole catalogue");
    } else
        CHECK_ARG(exclude_mode >= SBR_EVAL_EXCL_NONE && exclude_mode <= SBR_EVAL_EXCL_WINDOW,
                  "the LISTS road takes SBR_EVAL_EXCL_NONE, _VIEWED or _WINDOW, not mode %d", exclude_mode);
    const Layout& y = h->lay;
    const int C = c->cfg.n_clusters;
    SbrEvalView v;
    int rc;
    if ((rc = cluster_fits_engine(c, h)) != SBR_OK) return rc;
    if ((rc = eval_check_args(h, d, users, n, k, v)) != SBR_OK) return rc;
    // once per call, before the chunk loop: the member lists (host sizes, Lmax) or the membership matrix of the current R
    if ((rc = product ? sbr_cluster_build_hard(c, 1) : sbr_cluster_build_lists(c)) != SBR_OK) return rc;
    const int B = y.B, N = y.N;
    const int lmax = product ? 0 : c->lmax, kk = product ? k : std::min(k, lmax);      // kk: the depth ranked in the cluster matrix
    // the restricted kernel applies to the LISTS road only; every other case reads full score rows
    const bool restricted = !product && cluster_rank_restricted(h);
    const bool full = whole || !restricted;
    // the whole-catalogue ranking scores the items fed 0.0 where the compiled test function of a margin model does (_exclude_mode)
    const int whole_mode = (product && exclude_mode == SBR_EVAL_EXCL_WINDOW && SBR_LOSS_IS_MARGIN(y.cfg.loss)) ? SBR_EVAL_EXCL_WINDOW_ZERO : exclude_mode;
    Carver cv;
    const size_t o_users = cv.take((size_t)n * sizeof(int)), o_csel = cv.take((size_t)n * sizeof(int)), o_size = cv.take((size_t)n * sizeof(int));
    const size_t o_use = cv.take((size_t)C * sizeof(int));
    const EvalRecords rw = carve_records(cv, whole, n, k, N, B), ri = carve_records(cv, inside, n, k, N, B);
    const size_t o_grp = cv.take(restricted ? sbr_crk_group_words(B, C) * sizeof(int) : 0);
    const size_t o_cs = cv.take((size_t)B * (product ? N : lmax) * sizeof(float));
    const RankWork w = carve_rank_work(cv, B, k, k > kRankSortLds);      // one working set for both rankings (kk <= k: sized for the deeper one)
    const size_t o_osc = cv.take((size_t)B * k * sizeof(float));
    const size_t o_pos = cv.take(product ? 0 : (size_t)B * kk * sizeof(int)), o_psc = cv.take(product ? 0 : (size_t)B * kk * sizeof(float));
    if ((rc = rank_scratch(h, cv.at)) != SBR_OK) return rc;
    char* S = (char*)h->rank_scratch;
    hipStream_t s = h->stream;
    const int* dusers = (const int*)(S + o_users);
    int* dcsel = (int*)(S + o_csel);
    float *cs = (float*)(S + o_cs), *osc = (float*)(S + o_osc);
    // (pageable host memory: the copy has left the caller's array when it returns)
    SBR_HIP(hipMemcpyAsync(S + o_users, users, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    if ((rc = clear_records(h, S, rw)) != SBR_OK || (rc = clear_records(h, S, ri)) != SBR_OK) return rc;
    if (cluster_use_host) SBR_HIP(hipMemsetAsync(S + o_use, 0, (size_t)C * sizeof(int), s));
    for (int64_t c0 = 0; c0 < n; c0 += B) {
        const int rows = (int)std::min<int64_t>(B, n - c0);
        const int* cu = dusers + c0;
        int* csel = dcsel + c0;
        if ((rc = eval_pack_chunk(h, v, cu, rows)) != SBR_OK) return rc;
        // (full: the very floats sbr_rank ranks)
        if ((rc = full ? full_scores(h, 0) : forward_current(h)) != SBR_OK) return rc;
        float* lg = h->A(y.a_logits);
        if ((rc = sbr_cluster_select(c, h_last(h), y.HLt, y.D == 2 ? y.HLp : 0, rows, csel, nullptr)) != SBR_OK) return rc;
        // --- the cluster ranking's scores, while the full scores are as the projection left them
        if (product)
            SBR_LAUNCH(launch_cev_product(s, v, cu, rows, y.T, N, C, exclude_mode == SBR_EVAL_EXCL_WINDOW, lg, csel, c->hardT, cs));
        else if ((rc = cluster_scores(c, h, S, o_grp, csel, rows, lmax, cs, restricted)) != SBR_OK) return rc;
        // --- the whole-catalogue ranking of the same forward pass: sbr_evaluate's chunk
        if (whole) {
            int* oid = rw.ids_at(S, c0);
            SBR_LAUNCH(launch_exclude(s, rows, ExclSources().dataset(v, cu, y.T, whole_mode), eval_sink(lg, N, whole_mode)));
            if ((rc = rank_rows(h, S, w, lg, rows, N, k, oid, osc)) != SBR_OK) return rc;
            if ((rc = launch_hits(h, S, rw, v, dusers, c0, rows, oid)) != SBR_OK) return rc;
        }
        // --- the cluster ranking
        int* oid = ri.ids_at(S, c0);
        if (product) {
            if ((rc = rank_rows(h, S, w, cs, rows, N, k, oid, osc)) != SBR_OK) return rc;
        } else {
            SBR_LAUNCH(launch_exclude(s, rows, ExclSources().dataset(v, cu, y.T, exclude_mode), ExclCluster{cs, lmax, csel, C, c->mem_ids, c->mem_off, N}));
            if ((rc = rank_rows(h, S, w, cs, rows, lmax, kk, (int*)(S + o_pos), (float*)(S + o_psc))) != SBR_OK) return rc;
            SBR_LAUNCH(launch_crk_translate(s, (const int*)(S + o_pos), (const float*)(S + o_psc), kk, k, csel, c->mem_ids, c->mem_off, rows,
                                            oid, osc, (int*)(S + o_size) + c0));
        }
        if ((rc = launch_hits(h, S, ri, v, dusers, c0, rows, oid)) != SBR_OK) return rc;
    }
    if (cluster_use_host) SBR_LAUNCH(launch_cev_use(s, dcsel, (long long)n, C, (int*)(S + o_use)));
    if (whole && (rc = fetch_records(h, S, rw)) != SBR_OK) return rc;
    if ((rc = fetch_records(h, S, ri)) != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(cluster_host, dcsel, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (size_host) SBR_HIP(hipMemcpyAsync(size_host, S + o_size, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (cluster_use_host) SBR_HIP(hipMemcpyAsync(cluster_use_host, S + o_use, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, s));
    return check_fault(h);          // a forward that gave up must not hand out rankings; the call's one wait for the device
}
