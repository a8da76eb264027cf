// Prints sbr_scat_plan (csrc/sbr_scatter.hip) over a fixed grid of shapes, one line per shape: the inputs, " | ", every field of the
// plan and the path of the counting sort in front of it.  Host code only -- no HIP call, runs without a GPU.
// tests/test_scat_plan_table.py builds it (make -C csrc scat_plan_table) and compares its output with
// tests/golden/scat_plan_table.txt, which the predicates of the commit named in that file's first line produced for the same grid:
// the ladders of layer0_scatter / backward_bi / backward_tail, the refusals of the launchers they tried, scat_lds_plan and the
// layout's slab rule, applied in that commit's order.
//
// The grid moves one input at a time off a base shape (3 706 ids, 51 200 entries, one direction, no embedding, the switches' defaults,
// no tail): every row width with every SBR_SCAT_RANGE, with and without its partial-row slab; from each width the flag, an
// embedding, two directions, the entry count, a slab one slot short, and a tail of 2 and of 8 chunks with both values of
// SBR_TAIL_SCATTER_LDS.  The id counts are those at which some width's LDS-row form stops fitting its 120 KB (found by asking the
// plan; every width up to 512 floats gets all of them) and those on both sides of the LDS histogram's key space.
#include "sbr_common.h"
#include <stdio.h>
#include <set>
#include <string>
#include <vector>

struct Row { int GHp = 384, n_ids = 3706, entries = 51200, Ep = 0, D = 1, atomic = 0, range = 1, lds = 1, tch = 0, slots = -1; };
// the partial-row slab as sbr_build_layout sizes it
static int slots_of(const Row& r) {
    if (r.slots >= 0) return r.slots;
    return sbr_scatter_wide_rows(r.Ep, r.GHp) ? std::max(sbr_scatter_wide_slots((size_t)r.entries), 2 * SBR_SCAT_RANGES) : 0;
}
struct Ans { int plain, tail, nv, comb, range_nv, wide_nvw, wide_nvb, poll_nv, lds_nv, floor_cost, rows_lds, wide_rows; };
static Ans answer(const Row& r) {
    const ScatPlan p = sbr_scat_plan(r.GHp, r.Ep, r.n_ids, r.entries, r.D, r.atomic != 0, r.range, r.lds, r.tch, kTailScatterUnits, slots_of(r));
    return {p.plain, p.tail, p.reduce.nv, p.reduce.comb, p.range_nv, p.wide_nvw, p.wide_nvb, p.poll_nv, p.lds_nv, p.floor_cost, p.rows_lds, p.wide_rows};
}

static std::set<std::string> seen;
static void emit1(const Row& r) {
    char in[160];
    snprintf(in, sizeof(in), "%d %d %d %d %d %d %d %d %d %d", r.GHp, r.n_ids, r.entries, r.Ep, r.D, r.atomic, r.range, r.lds, r.tch, slots_of(r));
    if (!seen.insert(in).second) return;
    const Ans a = answer(r);
    // the sort in front: plain keys in the LDS histogram (L) or aggregated (A); time-chunked keys fit the histogram (L) or the sort refuses (X)
    const long keys = (long)r.n_ids * (r.tch >= 2 ? r.tch : 1);
    const char sort = keys <= sbr_scatter_lds_ids() ? 'L' : r.tch >= 2 ? 'X' : 'A';
    const bool tail = r.tch >= 2;      // (no tail: its columns are not read)
    printf("%s | %d %c %d %d %d %d %d %d %d %d %d %d %c\n", in, a.plain, tail ? '0' + a.tail : '-', a.nv, a.comb, a.range_nv, a.wide_nvw, a.wide_nvb,
           tail ? a.poll_nv : 0, tail ? a.lds_nv : 0, tail ? a.floor_cost : 0, tail ? a.rows_lds : 0, a.wide_rows, sort);
}

int main() {
    printf("# GHp n_ids entries Ep D atomic scat_range tail_scatter_lds tail_chunks part_slots"
           " | plain tail reduce_nv reduce_comb range_nv wide_nvw wide_nvb poll_nv lds_nv floor_cost rows_lds wide_rows sort\n");
    const int widths[] = {64, 128, 256, 384, 512, 576, 768, 1024, 1040, 1536, 2048, 2304, 4096, 8192, 8208};
    // id counts at which the LDS-row form of some width stops fitting (2 tail chunks): the last that fits and the first that does not
    std::vector<int> flips;
    for (int GHp : widths) {
        Row r; r.GHp = GHp; r.tch = 2; r.n_ids = 1;
        if (answer(r).tail != SCAT_LDS) continue;
        int lo = 1, hi = 1 << 22;      // fits at lo, not at hi
        while (hi - lo > 1) { r.n_ids = (lo + hi) / 2; if (answer(r).tail == SCAT_LDS) lo = r.n_ids; else hi = r.n_ids; }
        flips.push_back(lo); flips.push_back(hi);
    }
    const int L = sbr_scatter_lds_ids();
    for (int GHp : widths) {
        Row b; b.GHp = GHp;
        auto with = [&](auto f) { Row r = b; f(r); emit1(r); };
        for (int range : {0, 1, 2}) { with([=](Row& r) { r.range = range; }); with([=](Row& r) { r.range = range; r.slots = 0; }); }
        with([](Row& r) { r.atomic = 1; });
        with([](Row& r) { r.Ep = 64; }); with([](Row& r) { r.Ep = 576; });
        with([](Row& r) { r.D = 2; });
        with([](Row& r) { r.entries = 384; }); with([](Row& r) { r.entries = 384; r.slots = 0; });
        // a slab with every slot the segment-parallel form may claim, and one slot short of them
        for (int d : {0, 1}) with([=](Row& r) { r.range = 2; r.entries = 204800; r.slots = sbr_scatter_wide_slots((size_t)r.entries) - d; });
        for (int tch : {2, 8}) {
            with([=](Row& r) { r.tch = tch; }); with([=](Row& r) { r.tch = tch; r.lds = 0; });
            for (int e : {384, 204800}) with([=](Row& r) { r.tch = tch; r.entries = e; });
        }
        if (GHp <= 512) for (int n : flips) with([=](Row& r) { r.tch = 2; r.n_ids = n; });
        if (GHp == 384)      // the key space of the LDS histogram from both sides, with plain and with time-chunked keys
            for (int tch : {0, 2, 8}) for (int k : {1, 2, 8}) for (int n : {L / k, L / k + 1}) with([=](Row& r) { r.tch = tch; r.n_ids = n; });
    }
    return 0;
}
