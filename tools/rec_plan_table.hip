// Prints sbr_rec_plan (csrc/sbr_rec.hip) over a fixed grid of layer shapes, one line per shape: the inputs, " | ", every field of
// the plan.  Host code only -- no HIP call, runs without a GPU.  tests/test_rec_plan_table.py builds it (make -C csrc plan_table)
// and compares its output with tests/golden/rec_plan_table.txt, which the predicates of the commit named in that file's first line
// produced, applied in the order its launchers and sbr_query applied them.
//
// The grid: base shapes (cell x padded width x rows per workgroup, everything else at the engine's defaults) and, from every base
// shape, one row per clause input moved off its default -- switches, flags, the pointers a kernel family asks for, the batch / time /
// vocabulary sizes on both sides of every byte bound of that shape -- plus a few pairs of them.  Rows that differ in one input
// only are what the test looks for: every value of every input column must change the plan somewhere.
#include "sbr_common.h"
#include <stdio.h>
#include <string.h>
#include <set>
#include <string>

struct Row {
    int cell = SBR_CELL_GRU, T = 12, Bp = 64, Hp = 128, n_in = 1000; float clip = 100.0f;
    int rpt = 4, pipe = 1, f16 = 1, f16b = 1, cl16 = 1, cluster = 1, f32 = 0, prof = 0, relu = 0;
    int contig = 1, xh = 1, pring = 1, goff = 0, dh_ext = 0, simple = 0, fused = 1;
};

// the shape as the engine would hand it over: arrays at made-up addresses whose DISTANCES are what the predicates read
static RecArgs args_of(const Row& r) {
    RecArgs a; memset(&a, 0, sizeof(a));
    a.cell = r.cell; a.T = r.T; a.Bp = r.Bp; a.H = r.Hp; a.Hp = r.Hp; a.G = sbr_gates(r.cell); a.n_in = r.n_in; a.clip = r.clip;
    a.rpt = r.rpt; a.x6_pipe = r.pipe; a.x6_f16 = r.f16; a.x6_f16_bwd = r.f16b; a.cl16 = r.cl16; a.c16_two_level = 1;
    a.cluster = r.cluster; a.f32_mfma = r.f32; a.relu = r.relu;
    char* base = (char*)((uintptr_t)1 << 44);
    a.hs = (float*)base; a.cs = (float*)(base + 1024);
    // goff 0: the saved gates behind hs / cs in reach of a 31-bit offset; 1: in front of them; 2: 2^31 bytes and more behind them
    char* g0 = r.goff == 1 ? base - ((size_t)1 << 40) : r.goff == 2 ? base + 1024 + ((size_t)1 << 31) : base + 2048;
    const size_t one = (size_t)r.T * r.Bp * r.Hp + (r.contig ? 0 : 64);
    for (int k = 0; k < 4; ++k) a.g[k] = (float*)g0 + (size_t)k * one;
    if (r.prof) a.prof = (unsigned long long*)(base - 4096);
    if (r.xh) a.xh = base - 8192;
    if (r.pring) a.pring = (float*)(base - 16384);
    if (r.dh_ext) a.dh_ext = (const float*)(base - 32768);
    return a;
}

static const char* kname(RecKernel k) {
    static const char* n[] = {"triage", "c16", "cl8", "x6p", "x6q", "x6s", "x6", "mfma"};
    return n[k];
}

static std::set<std::string> seen;
static void emit(const Row& r) {
    char in[256];
    snprintf(in, sizeof(in), "%d %d %d %d %d %g %d %d%d%d%d%d %d%d%d%d%d %d%d%d%d%d", r.cell, r.T, r.Bp, r.Hp, r.n_in, r.clip, r.rpt,
             r.pipe, r.f16, r.f16b, r.cl16, r.cluster, r.f32, r.prof, r.relu, r.simple, r.fused, r.contig, r.xh, r.pring, r.goff, r.dh_ext);
    if (!seen.insert(in).second) return;
    const RecPlan p = sbr_rec_plan(args_of(r), r.simple != 0, r.fused != 0);
    printf("%s | %s %s %d %d %d %d %d %d %d %d %d%d%d%d%d %zu %zu\n", in, kname(p.fwd), kname(p.bwd), p.family, p.fwd_rows, p.bwd_rows,
           p.fwd_wgs, p.bwd_wgs, p.products_fwd, p.products_bwd, p.bwd_blocks, (int)p.bwd_chunkable, (int)p.fuse_gather, (int)p.tail_ok,
           (int)p.needs_fill, p.bwd_dbuf, p.fwd_lds, p.bwd_lds);
}

static int ceil_div16(unsigned long long bound, unsigned long long per_row) {      // first multiple of 16 rows at or above bound bytes
    const unsigned long long n = (bound + per_row - 1) / per_row;
    return (int)((n + 15) / 16 * 16);
}

int main() {
    // (three groups of five one-digit inputs, one group of five one-digit outputs: the lines stay short)
    printf("# cell T Bp Hp n_in clip rpt x6_pipe,x6_f16,x6_f16_bwd,cl16,cluster f32_mfma,prof,relu,simple,fused contiguous,xh,pring,gate_offset,dh_ext"
           " | fwd bwd family fwd_rows bwd_rows fwd_wgs bwd_wgs products_fwd products_bwd bwd_blocks"
           " bwd_chunkable,fuse_gather,tail_ok,needs_fill,bwd_dbuf fwd_lds bwd_lds\n");
    const int cells[] = {SBR_CELL_LSTM, SBR_CELL_GRU, SBR_CELL_VANILLA};
    const int widths[] = {16, 32, 48, 64, 128, 256, 304, 512, 1024, 1040};
    const int rpts[] = {1, 2, 4, 8, 16};
    for (int cell : cells) for (int Hp : widths) for (int rpt : rpts) {
        const bool small = Hp == 32 || Hp == 64 || Hp == 128;      // the widths whose kernels come in several tile heights
        if (!small && rpt != 4) continue;
        Row b; b.cell = cell; b.Hp = Hp; b.rpt = rpt;
        emit(b);
        auto with = [&](auto f) { Row r = b; f(r); emit(r); };
        auto with2 = [&](auto f, auto g) { Row r = b; f(r); g(r); emit(r); };
        auto pipe0 = [](Row& r) { r.pipe = 0; };      auto f16_0 = [](Row& r) { r.f16 = 0; };
        auto f16b0 = [](Row& r) { r.f16b = 0; };      auto cl16_0 = [](Row& r) { r.cl16 = 0; };
        auto cluster0 = [](Row& r) { r.cluster = 0; }; auto f32 = [](Row& r) { r.f32 = 1; };
        auto prof = [](Row& r) { r.prof = 1; };       auto relu = [](Row& r) { r.relu = 1; };
        auto split = [](Row& r) { r.contig = 0; };    auto noxh = [](Row& r) { r.xh = 0; };
        auto nopring = [](Row& r) { r.pring = 0; };   auto ext = [](Row& r) { r.dh_ext = 1; };
        auto simple = [](Row& r) { r.simple = 1; };   auto unfused = [](Row& r) { r.fused = 0; };
        auto clip0 = [](Row& r) { r.clip = 0.0f; };   auto clip1000 = [](Row& r) { r.clip = 1000.0f; };
        with(pipe0); with(f16_0); with(f16b0); with(cl16_0); with(cluster0); with(f32); with(prof); with(relu); with(split); with(noxh);
        with(nopring); with(ext); with(simple); with(unfused); with(clip0); with(clip1000);
        with([](Row& r) { r.goff = 1; }); with([](Row& r) { r.goff = 2; });
        with([](Row& r) { r.Bp = 72; }); with([](Row& r) { r.Bp = 68; });      // a multiple of 8 that is none of 16; none of 8
        for (int T : {4095, 4096, 4097}) with([T](Row& r) { r.T = T; });
        with2(pipe0, f16b0); with2(cl16_0, f16b0);
        if (!small) continue;
        // the byte bounds: rows of W_in behind a 32-bit offset (fused gather), rows of the batch behind 32-bit offsets into the saved
        // activations / the four-gate element, the whole of dxt behind a 31-bit offset (overlapped tail)
        const unsigned long long G = sbr_gates(cell), p32 = 1ull << 32, p31 = 1ull << 31;
        const int n_lim = (int)((p32 + G * Hp * 4 - 1) / (G * Hp * 4));
        for (int n : {n_lim - 1, n_lim}) { with([n](Row& r) { r.n_in = n; }); with2([n](Row& r) { r.n_in = n; }, unfused); }
        // (at 128 units the bound on Bp * G * Hp * 4 lies behind the one on the 16-byte gate element for every cell, G <= 4: no row can
        // show it alone, so none tries)
        for (int d : {-16, 0}) {
            if (Hp != 128) with([&](Row& r) { r.Bp = ceil_div16(p32, G * Hp * 4) + d; });
            else {
                with([&](Row& r) { r.Bp = ceil_div16(p32, Hp * 16) + d; });
                with([&](Row& r) { r.Bp = ceil_div16(p31, 12 * G * Hp * 4) + d; });
            }
        }
    }
    return 0;
}
