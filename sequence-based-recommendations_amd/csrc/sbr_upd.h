// K13, the optimizer rule, once: lasagne.updates.{adagrad,rmsprop,adadelta,nesterov_momentum,adam} [3P] (update_manager.py:24-82)
// with their epsilons, Adam's step size, and the hyperparameters every step kernel takes.  Host and device: the dense kernels
// (sbr_update.hip) and the row-sparse one (sbr_sparse.hip) call upd_step on registers; tools/upd_rule_table.hip runs it on the CPU
// (tests/test_upd_rule_table.py holds it bit for bit to a NumPy float32 transcription, and that to the float64 oracle).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/sbr_rnn.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// a_t: Adam's step size of step t; 0 for the other updaters
struct SbrUpdRule { int updater; float lr, rho, b1, b2, a_t; };

// a_t = lr sqrt(1 - b2^t) / (1 - b1^t) in double, rounded to float: the one place the expression stands.  The lazy catch-up of the
// row-sparse path replays missed steps from a table of these (sbr_api.hip) and is exact only while the dense launches use the same.
static inline double sbr_adam_at_d(double lr, double b1, double b2, long t) { return lr * sqrt(1.0 - pow(b2, (double)t)) / (1.0 - pow(b1, (double)t)); }
static inline float sbr_adam_at(double lr, double b1, double b2, long t) { return (float)sbr_adam_at_d(lr, b1, b2, t); }

// the rule of step t (t counts from 1)
static inline SbrUpdRule sbr_upd_rule(int updater, float lr, float rho, float b1, float b2, long t) {
    return {updater, lr, rho, b1, b2, updater == SBR_UPD_ADAM ? sbr_adam_at(lr, b1, b2, t) : 0.0f};
}
static inline SbrUpdRule sbr_upd_rule(const sbr_config& c, long t) { return sbr_upd_rule(c.updater, c.learning_rate, c.rho, c.beta1, c.beta2, t); }

// One element's step on registers: g = its gradient; p, s0, s1 = parameter and optimizer state, stepped in place.  adagrad, rmsprop
// and nesterov leave s1 as it is (they have one state array: the caller holds a 0 there and does not store it).
__host__ __device__ __forceinline__ void upd_step(const SbrUpdRule& st, float g, float& p, float& s0, float& s1) {
    switch (st.updater) {
        case SBR_UPD_ADAGRAD: { const float acc = s0 + g * g; s0 = acc; p -= st.lr * g / sqrtf(acc + 1e-6f); return; }
        case SBR_UPD_RMSPROP: { const float acc = st.rho * s0 + (1.0f - st.rho) * g * g; s0 = acc; p -= st.lr * g / sqrtf(acc + 1e-6f); return; }
        case SBR_UPD_ADADELTA: {
            const float acc = st.rho * s0 + (1.0f - st.rho) * g * g;
            const float upd = g * sqrtf(s1 + 1e-6f) / sqrtf(acc + 1e-6f);
            s0 = acc; p -= st.lr * upd; s1 = st.rho * s1 + (1.0f - st.rho) * upd * upd; return;
        }
        case SBR_UPD_NESTEROV: { const float v = st.rho * s0 - st.lr * g; s0 = v; p += st.rho * v - st.lr * g; return; }    // sgd + apply_nesterov_momentum
        default: {                                                                                                          // adam, eps 1e-8
            const float m = st.b1 * s0 + (1.0f - st.b1) * g;
            const float v = st.b2 * s1 + (1.0f - st.b2) * g * g;
            s0 = m; s1 = v; p -= st.a_t * m / (sqrtf(v) + 1e-8f); return;
        }
    }
}
// ... of a 16-byte piece
__host__ __device__ __forceinline__ void upd_step4(const SbrUpdRule& st, const f32x4& g, f32x4& p, f32x4& s0, f32x4& s1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { float pe = p[e], ae = s0[e], be = s1[e]; upd_step(st, g[e], pe, ae, be); p[e] = pe; s0[e] = ae; s1[e] = be; }
}
