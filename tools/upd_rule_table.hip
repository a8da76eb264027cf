// Prints upd_step (csrc/sbr_upd.h) over a fixed grid, one line per row: updater, hyperparameter set, t, the inputs g p s0 s1, " | ",
// a_t and the stepped p s0 s1, every float as a hex float.  Host code only -- no HIP call, no link against the library, runs without
// a GPU.  tests/test_upd_rule_table.py builds it (make -C csrc upd_rule_table) and compares every row bit for bit with a NumPy
// float32 transcription of the rule.
//
// The grid: five updaters x two hyperparameter sets (the defaults; lr 0.05, rho 0.8, beta1 0.7, beta2 0.95) x 320 draws of
// (g, p, s0, s1, t) from a fixed LCG.  Magnitudes are 2^e (1 + u): g over e in [-10, 1], p over [-6, 2], the state arrays over
// [-14, 2]; every 16th draw has g == 0 (the step the lazy catch-up replays), every 20th starts from zero state (the first step).
// s0 keeps its sign where it is a velocity or a first moment (nesterov, adam) and is an accumulator (>= 0) elsewhere; s1 >= 0.  t is
// small (1 .. 64) in half of the draws and 2^(1 .. 16.3) in the rest: past the step from which a_t == (float)lr with either set.
#include "sbr_upd.h"
#include <stdint.h>
#include <stdio.h>

static uint32_t lcg_state = 20241u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }       // 24 bits
static float unit() { return (float)lcg() / 16777216.0f; }                                            // [0, 1), exact
static float mag(int e_lo, int e_hi) { const int e = e_lo + (int)(lcg() % (uint32_t)(e_hi - e_lo + 1)); return ldexpf(1.0f + unit(), e); }
static float sign() { return (lcg() & 1) ? -1.0f : 1.0f; }

int main() {
    const float sets[2][4] = {{0.01f, 0.9f, 0.9f, 0.999f}, {0.05f, 0.8f, 0.7f, 0.95f}};      // lr, rho, beta1, beta2
    const int updaters[5] = {SBR_UPD_ADAGRAD, SBR_UPD_RMSPROP, SBR_UPD_ADADELTA, SBR_UPD_NESTEROV, SBR_UPD_ADAM};
    printf("# updater set t g p s0 s1 | a_t p s0 s1\n");
    for (int d = 0; d < 320; ++d) {
        float g = sign() * mag(-10, 1), p = sign() * mag(-6, 2), s0 = sign() * mag(-14, 2), s1 = mag(-14, 2);
        long t = (d & 1) ? 1 + (long)(lcg() % 64u) : (long)exp2(1.0 + 15.3 * (double)unit());
        if (d == 0) t = 1;
        if (d % 16 == 5) g = 0.0f;
        if (d % 20 == 7) { s0 = 0.0f; s1 = 0.0f; }
        for (int u : updaters)
            for (int h = 0; h < 2; ++h) {
                const SbrUpdRule st = sbr_upd_rule(u, sets[h][0], sets[h][1], sets[h][2], sets[h][3], t);
                const float a = (u == SBR_UPD_NESTEROV || u == SBR_UPD_ADAM) ? s0 : fabsf(s0);
                float pe = p, ae = a, be = s1;
                upd_step(st, g, pe, ae, be);
                printf("%d %d %ld %a %a %a %a | %a %a %a %a\n", u, h, t, g, p, a, s1, st.a_t, pe, ae, be);
            }
    }
    return 0;
}
