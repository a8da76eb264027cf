// Prints sbr_gemm_plan (csrc/sbr_gemm.hip) over a fixed grid, one line per row: the inputs, " | ", every field of the plan.  Host code
// only -- no HIP call, runs without a GPU.  tests/test_gemm_plan_table.py builds it (make -C csrc gemm_plan_table) and compares its
// output with tests/golden/gemm_plan_table.txt, which the launchers of the commit named in that file's first line produced: their
// ladder ran with every kernel launch replaced by a record of what it would have launched.
//
// The grid: the six modes of sbr_debug_gemm crossed with M and N on both sides of every threshold of the ladder (M beside a large
// N, N beside a large M, both together) at a short and a long K, and with K on both sides of its thresholds at three of those
// shapes; without a workspace, with one of M * N floats (no room for a split) and with an ample one, there with a bias and with a
// consumer that keeps the slabs; the modes an engine builds that sbr_debug_gemm cannot name, on a thinner grid; tile counts on both
// sides of the 128-workgroup switches of the 128 x 128 and the 256 x 128 tile; operands the tiled kernel does not read (blocked,
// misaligned, no unit stride) and the ones the wide tile leaves to the 128-wide kernel (A transposed, an output that is not 16-byte
// aligned).
#include "sbr_common.h"
#include <stdio.h>

struct Mode { const char* name; GemmMode m; };
//                                       simple exact planes sa sb no_wide one_pass
static const Mode kDebug[] = {{"0", {false, false, 0, 1.0f, 1.0f, false, false}}, {"1", {false, true, 0, 1.0f, 1.0f, false, false}},
                              {"2", {false, false, 0, 1.0f, 1.0f, false, true}},  {"3", {false, false, 2, 1.0f, 1.0f, false, false}},
                              {"4", {false, false, 2, 1.0f, 1.0f, true, false}},  {"5", {false, false, 0, 1.0f, 1.0f, true, true}}};
// simple; scores under SBR_FLAG_BF16_PROJECTION; SBR_FLAG_BF16_LAYERS without and with SBR_FLAG_F32_MFMA; a gradient on either
// side of the fp16 split; bf16x6 stated (the weight-gradient slabs' mode); the split under SBR_FLAG_F32_MFMA
static const Mode kEngine[] = {{"simple", {true, false, 2, 1.0f, 1.0f, false, true}},  {"scores1", {false, true, 0, 1.0f, 1.0f, false, true}},
                               {"layers1", {false, false, 1, 1.0f, 1.0f, false, false}}, {"layers1e", {false, true, 1, 1.0f, 1.0f, false, false}},
                               {"gradA", {false, false, 2, 512.0f, 1.0f, false, false}}, {"gradB", {false, false, 2, 1.0f, 512.0f, false, false}},
                               {"x6", {false, false, 3, 1.0f, 1.0f, false, false}},      {"f16e", {false, true, 2, 1.0f, 1.0f, false, false}}};

// operands at made-up addresses; layout r: row-major, t: transposed, b: blocked, m: row-major 4 bytes off a 16-byte boundary,
// o: row-major with an odd leading dimension, s: no unit stride
static GemmOperand operand(char layout, char* base, long ld) {
    const float* p = (const float*)base;
    switch (layout) {
        case 't': return gemm_transposed(p, ld);
        case 'b': return GemmOperand{p, ld, 1, 16};
        case 'm': return gemm_rowmajor(p + 1, ld);
        case 'o': return gemm_rowmajor(p, ld + 1);
        case 's': return GemmOperand{p, 2 * ld, 2, 0};
        default: return gemm_rowmajor(p, ld);
    }
}

// ws: 0 none, 1 M * N floats, 2 ample.  c: 0 an aligned output with ldc = N, 1 ldc = N + 1
static void emit(const Mode& md, int M, int N, int K, int bias, int ws, int keep, char a, char b, int c) {
    char* base = (char*)((uintptr_t)1 << 44);
    const GemmOperand A = operand(a, base, a == 't' ? M : K), B = operand(b, base + ((size_t)1 << 40), b == 't' ? K : N);
    const float* C = (const float*)(base + ((size_t)2 << 40));
    const float* W = ws ? (const float*)(base + ((size_t)3 << 40)) : nullptr;
    const size_t ws_floats = ws == 1 ? (size_t)M * N : ws == 2 ? (size_t)1 << 28 : 0;
    const GemmPlan p = sbr_gemm_plan(md.m, A, B, C, N + c, M, N, K, bias != 0, W, ws_floats, keep != 0);
    static const char* kn[] = {"naive", "x6", "f32"};
    printf("%s %d %d %d %d%d%d %c%c%d | %s %d %d %d %d %g %g %d%d\n", md.name, M, N, K, bias, ws, keep, a, b, c, kn[p.kernel], p.tile, p.nsplit,
           p.kchunk, p.planes, p.sa, p.sb, (int)p.reduce, (int)p.keep);
}
// the workspace / bias / consumer combinations of one shape: none; where K is long enough for the f32 kernel to split it, a workspace
// of M * N floats (no room for a split) and an ample one; where the tiled kernel splits too, a consumer that keeps the slabs, without
// and with a bias
static void emit_ws(const Mode& md, int M, int N, int K, char a = 'r', char b = 'r', int c = 0) {
    emit(md, M, N, K, 0, 0, 0, a, b, c);
    if (K >= 128) { emit(md, M, N, K, 0, 1, 0, a, b, c); emit(md, M, N, K, 0, 2, 0, a, b, c); }
    if (K >= 512) { emit(md, M, N, K, 0, 2, 1, a, b, c); emit(md, M, N, K, 1, 2, 1, a, b, c); }
}

int main() {
    printf("# mode M N K bias,ws,keep_allowed layoutA,layoutB,ldc_odd | kernel tile nsplit kchunk planes sa sb reduce,keep\n");
    // M beside N = 1024, N beside M = 1024, and both together, at the shortest K the tiled kernel takes and at a long one; every K on
    // both sides of its thresholds (32: the tiled kernel, 128: the f32 kernel's split, 512: the tiled kernel's) at three of the shapes
    const int edge[] = {47, 48, 95, 96, 128, 1024};
    for (int m = 0; m < 6; ++m)
        for (int M : edge) for (int N : edge) {
            if (M != 1024 && N != 1024 && M != N) continue;
            if (m >= 4 && M != N && M != 1024) continue;      // (modes 4 / 5 differ from 3 / 2 on the wide tile only, 256 rows and more)
            const bool all_k = (M == 96 && N == 96) || (M == 1024 && N == 1024) || (M == 47 && N == 1024 && m < 4);
            for (int K : {31, 32, 127, 128, 511, 512, 4096}) if (all_k || K == 32 || K == 4096) emit_ws(kDebug[m], M, N, K);
        }
    for (const Mode& md : kEngine)
        for (const auto& s : {edge + 0, edge + 3, edge + 5}) for (int K : {32, 4096}) { emit_ws(md, *s, *s, K); if (*s == 47) emit_ws(md, 47, 1024, K); }
    // 121 / 132 tiles of 128 x 128; 112 / 120 / 128 / 256 tiles of 256 x 128 (and what a split adds to them)
    const int big[][2] = {{1408, 1408}, {1536, 1408}, {1792, 2048}, {2048, 1920}, {2048, 2048}, {4096, 2048}, {2048, 2000}, {2040, 2048}};
    for (const Mode& md : kDebug)
        for (const auto& s : big) for (int K : {480, 512, 4096}) for (int w : {0, 2}) if (K != 480 || !w) emit(md, s[0], s[1], K, 0, w, w / 2, 'r', 'r', 0);
    for (const Mode& md : kEngine)
        for (const auto& s : {big[1], big[4], big[7]}) for (int w : {0, 2}) emit(md, s[0], s[1], 1024, 0, w, w / 2, 'r', 'r', 0);
    // the operands: the layouts of the step (r / t on either side) and the ones only the f32 kernel reads
    for (const Mode& md : kDebug)
        for (const char* l : {"tr0", "rt0", "tt0", "br0", "rb0", "mr0", "rm0", "or0", "ro0", "sr0", "rs0", "rr1", "tr1"})
            for (int w : {0, 2}) emit(md, 2048, 2048, 1024, 0, w, w / 2, l[0], l[1], l[2] - '0');
    return 0;
}
