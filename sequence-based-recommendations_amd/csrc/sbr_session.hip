// Stateful sessions (include/sbr_rnn.h "Stateful sessions"; DESIGN.md sections 3o and 3r): a pool of kept recurrent states beside the
// engine, one recurrent step per event.  sbr_sessions_create / destroy / reset / advance / replay / adopt / read / write and their kernels; the
// ranking call sbr_sessions_rank is an entry to sbr_rank's pipeline and lives with it (sbr_rank_api.hip).  Parking -- the record of a
// session off the device, sbr_sessions_record_layout / export / import and their two kernels -- is at the end.
//
// The step (ses_step_kernel; its tile computation, ses_tile, is shared with ses_replay_kernel below), one launch per layer: for the
// rows r < n of a call, s = slots[r],
//     x = input(r) . W_in + b        layer 0 with index input: b + the F gathered rows of W_in (gather_xt_kernel's order);
//                                    --r_emb: the F gathered embedding rows, flattened, as the A operand; layer >= 1: the lower
//                                    layer's NEW state of slot s
//     a = h[s] . W_hid               K = Hp
//     cell_forward<CELL>(x, a, ...)  sbr_cell.h: the chains' cell math, libm transcendentals
// on v_mfma_f32_16x16x4_f32 (exact f32 products).  A wave owns 16 rows x 16 units x G gates, x and a in accumulators of their own
// (GRU's candidate is x_c + r * a_c).  Lane (q, j) of the instruction supplies A[row j][k] and B[k][unit j] for the k of its group q
// and receives D[row 4q + e][unit j]; the wave walks K in blocks of 16, lane group q loading the quad k0 + 4q .. + 3 of its row with
// one 16-byte load, so the e-th instruction of a block sums k0 + e, + 4, + 8, + 12.  An output element is therefore ONE accumulation
// chain over K in an order fixed by K alone: it depends on its own row of A and column of B, never on which rows share the tile or
// the launch (tests/test_gpu_sessions.py holds the kernel to that, bit for bit).  Operands come straight from global memory: the
// step is launch- and latency-bound (4 096 sessions at 128 units: 0.4 GFLOP; W_hid stays in L2), and one arithmetic serves every
// cell, width and flag.
//
// Geometry: grid (ceil(Hp / 64), ceil(n / 16)), 256 threads = 4 waves = 4 unit tiles of one row tile; no LDS, no barrier.  16 rows
// at 48 units: 1 workgroup; 4 096 rows at 128 units: 512.
//
// The in-place hazard: the workgroups of different unit tiles all read the whole h[s], so no one may overwrite it.  Every slot has
// two planes per layer; a step reads plane (events[s] & 1) and writes the other, layer l + 1 reads layer l's written plane, and the
// commit launch behind the last layer counts the event -- which is what makes the written planes current.  Nothing reads a plane
// that a launch in flight writes: race-free by construction, given that the slots of a call are distinct (checked on the host).
#include "sbr_common.h"
#include "sbr_cell.h"
#include <algorithm>
#include <cstring>
#include <new>

namespace {

enum SesInput { SES_IN_INDEX = 0, SES_IN_EMB = 1, SES_IN_DENSE = 2 };

// one layer as the tile computation reads it
struct SesLayer {
    long long capacity;
    int Hp, K_in;                      // units of the layer; K of the dense input (F * Ep, or the lower layer's Hp)
    const float *Whid, *Win, *bias, *peep;
    float *hs, *cs;                    // this layer's planes
    const float* emb; int Ep;          // SES_IN_EMB: the embedding table [input_size][Ep]
    const float* in_hs; int in_Hp;     // SES_IN_DENSE: the lower layer's planes
    int relu;
};
// a row of the tile as a lane sees it: is it fed an event now, its slot, the events it had BEFORE this one (the plane to read:
// ev & 1), the ids fed (layer 0)
struct SesRowIn { bool ok; int s; long long ev; int id0, id1; };

// The tile computation of one layer and one event, shared by ses_step_kernel and ses_replay_kernel -- one arithmetic, so that the two
// leave the same bits: 16 rows x the 16 units from u0 x G gates by one wave.  ra: the row this lane supplies to operand A (row j of
// the tile), rm[e]: the rows whose results it holds (rows 4q + e).  A row that is not ok is computed as zeros and not written.
// U: the K blocks whose operands are loaded before the first of their instructions is issued.  The instructions and their order are
// the same for every U -- an output element stays the one chain over K --; only how many loads are in flight differs.  The step
// takes U = 1 (its launch hides nothing else either); the replay, whose every event waits for this walk, keeps ~60 loads in flight.
template <int CELL, int IN, int U>
__device__ __forceinline__ void ses_tile(const SesLayer& a, const int u0, const int j, const int q, const SesRowIn& ra,
                                         const SesRowIn (&rm)[4], const bool has_second) {
    constexpr int G = Gates<CELL>::G;
    const int Hp = a.Hp, GHp = G * Hp;
    const size_t plane = (size_t)a.capacity * Hp;
    const bool a_ok = ra.ok;
    const int sa = ra.s;
    const long long ea = ra.ev;
    const float* hrow = a.hs + (size_t)(ea & 1) * plane + (size_t)sa * Hp;
    f32x4 acc_a[G], acc_x[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { acc_a[g] = f32x4{0, 0, 0, 0}; acc_x[g] = f32x4{0, 0, 0, 0}; }
    // what the cell reads besides the two products, asked for before the walk over K so that it arrives behind it: the unit's
    // peepholes and biases, the rows' old state, the gathered rows of an index input
    const int u = u0 + j;
    float pi = 0.0f, pf = 0.0f, po = 0.0f;
    if (CELL == CELL_LSTM) { pi = a.peep[u]; pf = a.peep[Hp + u]; po = a.peep[2 * Hp + u]; }
    float b[G];
#pragma unroll
    for (int g = 0; g < G; ++g) b[g] = a.bias[g * Hp + u];
    float h_old[4], c_old[4], x0[4][G], x1[4][G];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h_old[e] = c_old[e] = 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) x0[e][g] = x1[e][g] = 0.0f;
        if (!rm[e].ok) continue;
        const size_t rd = (size_t)(rm[e].ev & 1) * plane + (size_t)rm[e].s * Hp + u;
        h_old[e] = a.hs[rd];
        if (CELL == CELL_LSTM) c_old[e] = a.cs[rd];
        if (IN == SES_IN_INDEX) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                x0[e][g] = a.Win[(size_t)rm[e].id0 * GHp + g * Hp + u];
                if (has_second) x1[e][g] = a.Win[(size_t)rm[e].id1 * GHp + g * Hp + u];
            }
        }
    }
    const unsigned col = (unsigned)(u0 + j);               // 32-bit element offsets from the uniform bases: W_hid and a dense W_in have far fewer than 2^31 elements
    // a group = U blocks of K: its operands are asked for (ld), then its instructions issued in the order of K (mm)
    auto ld = [&](const int k0, f32x4 (&hv)[U], float (&wv)[U][4][G]) {
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int kq = k0 + 16 * i + 4 * q;
            hv[i] = f32x4{0, 0, 0, 0};
            if (U > 1 && k0 + 16 * i >= Hp) continue;      // (uniform)
            if (a_ok) hv[i] = *(const f32x4*)(hrow + kq);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int g = 0; g < G; ++g) wv[i][e][g] = a.Whid[(unsigned)(kq + e) * (unsigned)GHp + (unsigned)(g * Hp) + col];
        }
    };
    auto mm = [&](const int k0, const f32x4 (&hv)[U], const float (&wv)[U][4][G]) {
#pragma unroll
        for (int i = 0; i < U; ++i) {
            if (U > 1 && k0 + 16 * i >= Hp) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int g = 0; g < G; ++g) acc_a[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[i][e], wv[i][e][g], acc_a[g], 0, 0, 0);
        }
    };
    if (U == 1) {
        for (int k0 = 0; k0 < Hp; k0 += 16) {
            f32x4 hv[U]; float wv[U][4][G];
            ld(k0, hv, wv);
            mm(k0, hv, wv);
        }
    } else {
        // two groups in flight: the next group's operands are asked for before this group's instructions issue, so that the matrix
        // pipe works while they travel
        f32x4 hv0[U], hv1[U]; float wv0[U][4][G], wv1[U][4][G];
        ld(0, hv0, wv0);
        for (int k0 = 0; k0 < Hp; k0 += 32 * U) {
            const int k1 = k0 + 16 * U, k2 = k0 + 32 * U;
            if (k1 < Hp) ld(k1, hv1, wv1);
            mm(k0, hv0, wv0);
            if (k1 < Hp) {
                if (k2 < Hp) ld(k2, hv0, wv0);
                mm(k1, hv1, wv1);
            }
        }
    }
    if (IN != SES_IN_INDEX) {
        const int K = a.K_in;                          // a multiple of 4: a quad is inside or outside
        const float* in_row = nullptr;
        if (IN == SES_IN_DENSE) in_row = a.in_hs + (size_t)((ea + 1) & 1) * ((size_t)a.capacity * a.in_Hp) + (size_t)sa * a.in_Hp;
        const int id0 = ra.id0, id1 = ra.id1;
        for (int k0 = 0; k0 < K; k0 += 16 * U) {
            f32x4 xv[U]; float wv[U][4][G];
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int kq = k0 + 16 * i + 4 * q;
                const bool in = kq < K;
                xv[i] = f32x4{0, 0, 0, 0};
                if (U > 1 && k0 + 16 * i >= K) continue;      // (uniform)
                if (a_ok && in) {
                    if (IN == SES_IN_DENSE) xv[i] = *(const f32x4*)(in_row + kq);
                    else { const int f = kq / a.Ep; xv[i] = *(const f32x4*)(a.emb + (size_t)(f ? id1 : id0) * a.Ep + (kq - f * a.Ep)); }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < G; ++g) wv[i][e][g] = in ? a.Win[(unsigned)(kq + e) * (unsigned)GHp + (unsigned)(g * Hp) + col] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < U; ++i) {
                if (U > 1 && k0 + 16 * i >= K) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < G; ++g) acc_x[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i][e], wv[i][e][g], acc_x[g], 0, 0, 0);
            }
        }
    }
    asm volatile("s_nop 15");                          // MFMA D -> VALU read hazard across the loop exit (see sbr_rec.hip)
    // the cell: this lane holds rows 4q + e of unit u
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!rm[e].ok) continue;
        const size_t wr = (size_t)((rm[e].ev + 1) & 1) * plane + (size_t)rm[e].s * Hp + u;
        float x[G], av[G], sv[4];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            av[g] = acc_a[g][e];
            if (IN == SES_IN_INDEX) {
                float v = b[g] + x0[e][g];
                if (has_second) v += x1[e][g];
                x[g] = v;
            } else
                x[g] = acc_x[g][e] + b[g];
        }
        float h = h_old[e], c = c_old[e];
        cell_forward<CELL>(x, av, true, h, c, pi, pf, po, sv, a.relu != 0);
        a.hs[wr] = h;
        if (CELL == CELL_LSTM) a.cs[wr] = c;
    }
}

struct SesStep {
    int n; const int* slots; const long long* events;
    SesLayer ly;
    const int *items, *second;         // layer 0: the ids fed (second: NULL with one index per step)
};

template <int CELL, int IN>
__global__ void __launch_bounds__(256) ses_step_kernel(SesStep a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const int u0 = (blockIdx.x * 4 + wave) * 16;
    if (u0 >= a.ly.Hp) return;                         // (no barrier in this kernel)
    const int r0 = blockIdx.y * 16;
    const bool ids = IN != SES_IN_DENSE;
    auto row = [&](int m) {
        SesRowIn r{m < a.n, 0, 0, 0, 0};
        if (r.ok) {
            r.s = a.slots[m]; r.ev = a.events[r.s];
            if (ids) { r.id0 = a.items[m]; r.id1 = a.second ? a.second[m] : 0; }
        }
        return r;
    };
    const SesRowIn ra = row(r0 + j);
    const SesRowIn rm[4] = {row(r0 + 4 * q), row(r0 + 4 * q + 1), row(r0 + 4 * q + 2), row(r0 + 4 * q + 3)};
    ses_tile<CELL, IN, 1>(a.ly, u0, j, q, ra, rm, a.second != nullptr);
}

// The replay (sbr_sessions_replay): the time loop and the layer loop of a run of events inside ONE launch.  A workgroup owns the 16
// rows of blockIdx.x (the rows of a call arrive longest first, so a tile's rows end together) and every unit tile of every layer:
// wave w walks the unit tiles w, w + 4, ... with ses_tile, the step's own arithmetic.  Between events and layers the states are
// exchanged through the slots' own two planes in global memory, exactly as a sequence of advance calls leaves them: event t of a row
// that had e0 events reads plane (e0 + t) & 1 and writes the other, so the final state lies in plane (e0 + len) & 1 with nothing
// copied.  A workgroup barrier behind every layer orders the planes' writes before their reads (all of them by this workgroup:
// workgroup scope); layer 0 of event t + 1 overwrites the plane layer 0 read at event t and nobody reads any more.  No workgroup
// waits for another.  A row whose list has ended is frozen: not computed, not written.  At the end the same launch counts the events
// and writes the ring, as len commit launches would have.
//
// TRACE (sbr_sessions_replay_ranks): the same kernel also writes the top layer's state BEFORE event t of row m to
// trace[trows[m].at + t][0 .. Hp_top), the rows sbr_sessions_rank would have projected at that moment.  At the head of iteration t the
// workgroup copies, for its rows that have an event t, the top layer's plane (e0 + t) & 1: the slot's current plane for t == 0, and
// for t >= 1 the plane the top layer wrote at event t - 1, behind that event's last layer barrier.  No barrier is added: that plane
// is next written by the top layer at event t + 1, behind the L >= 1 barriers that end iteration t (with L == 1 the top layer is
// layer 0, which in iteration t itself writes the OTHER plane), and a wave's loads have returned when it passes a barrier.  The state
// after the last event is not traced.  The TRACE = false instantiation holds none of this.
struct SesReplay {
    int n, L; const SesRow* rows; const int *items, *second;
    long long* events; int* ring; int ring_len;
    SesLayer ly[SBR_MAX_LAYERS];
    const SesTraceRow* trows; float* trace;          // TRACE only
};

template <int CELL, int IN, bool TRACE>
__global__ void __launch_bounds__(256) ses_replay_kernel(SesReplay a) {
    constexpr int U = CELL == CELL_VANILLA ? 4 : 2;    // 4 * G loads per K block, two groups of U blocks in flight: 32 to 64 loads
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.x * 16;
    const SesRow none{0, 0, 0};
    const int ma = r0 + j;
    const SesRow rowa = ma < a.n ? a.rows[ma] : none;
    const long long ea0 = ma < a.n ? a.events[rowa.slot] : 0;
    SesRow rowm[4]; long long em0[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int m = r0 + 4 * q + e;
        rowm[e] = m < a.n ? a.rows[m] : none;
        em0[e] = m < a.n ? a.events[rowm[e].slot] : 0;
    }
    const long long T = a.rows[r0].len;                // the longest row of the tile
    const bool has_second = a.second != nullptr;
    // TRACE: row (thread / 16) of the tile is copied by 16 threads, a 16-byte access each per 64 units
    const int mc = r0 + (threadIdx.x >> 4);
    SesRow rowc = none; long long ec0 = 0; float* tr = nullptr;
    if (TRACE && mc < a.n) {
        rowc = a.rows[mc]; ec0 = a.events[rowc.slot];
        tr = a.trace + (size_t)a.trows[mc].at * a.ly[a.L - 1].Hp;
    }
    for (long long t = 0; t < T; ++t) {
        if (TRACE && t < rowc.len) {
            const SesLayer& top = a.ly[a.L - 1];
            const float* src = top.hs + (size_t)((ec0 + t) & 1) * ((size_t)top.capacity * top.Hp) + (size_t)rowc.slot * top.Hp;
            float* dst = tr + (size_t)t * top.Hp;
            for (int u = (threadIdx.x & 15) * 4; u < top.Hp; u += 64) *(f32x4*)(dst + u) = *(const f32x4*)(src + u);
        }
        SesRowIn ra{t < rowa.len, rowa.slot, ea0 + t, 0, 0}, rm[4];
        if (ra.ok) { ra.id0 = a.items[rowa.start + t]; ra.id1 = has_second ? a.second[rowa.start + t] : 0; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            rm[e] = SesRowIn{t < rowm[e].len, rowm[e].slot, em0[e] + t, 0, 0};
            if (rm[e].ok) { rm[e].id0 = a.items[rowm[e].start + t]; rm[e].id1 = has_second ? a.second[rowm[e].start + t] : 0; }
        }
        for (int l = 0; l < a.L; ++l) {
            const SesLayer& ly = a.ly[l];
            for (int u0 = wave * 16; u0 < ly.Hp; u0 += 64) {
                if (l == 0) ses_tile<CELL, IN, U>(ly, u0, j, q, ra, rm, has_second);
                else ses_tile<CELL, SES_IN_DENSE, U>(ly, u0, j, q, ra, rm, false);
            }
            __syncthreads();
        }
    }
    // the commit: row (thread / 16) of the tile, its last min(len, ring_len) ids by 16 threads (T >= 1: the barriers above lie
    // between every read of events[] and this write; T == 0: nothing to write)
    const int m = r0 + (threadIdx.x >> 4);
    if (m >= a.n) return;
    const SesRow row = a.rows[m];
    if (row.len == 0) return;
    const long long e0 = a.events[row.slot];
    for (long long t = max(0ll, row.len - a.ring_len) + (threadIdx.x & 15); t < row.len; t += 16)
        a.ring[(size_t)row.slot * a.ring_len + (int)((e0 + t) % a.ring_len)] = a.items[row.start + t];
    if ((threadIdx.x & 15) == 0) a.events[row.slot] = e0 + row.len;
}

// behind the last layer: the event is counted (the planes the step wrote become the current ones) and its id enters the ring
__global__ void __launch_bounds__(256) ses_commit_kernel(SesPool p, const int* __restrict__ slots, const int* __restrict__ items, int n) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int s = slots[r];
    const long long e = p.events[s];
    p.ring[(size_t)s * p.ring_len + (int)(e % p.ring_len)] = items[r];
    p.events[s] = e + 1;
}

struct SesInit { const float* hinit[SBR_MAX_LAYERS]; const float* cinit[SBR_MAX_LAYERS]; };
// slot blockIdx.x of the list (slots NULL: slot blockIdx.x itself): plane 0 of every layer = the initial states as they are now, no events
__global__ void __launch_bounds__(256) ses_reset_kernel(SesPool p, SesInit in, const int* __restrict__ slots) {
    const long long s = slots ? slots[blockIdx.x] : blockIdx.x;
    for (int l = 0; l < p.L; ++l)
        for (int u = threadIdx.x; u < p.Hp[l]; u += 256) {
            p.hs[l][(size_t)s * p.Hp[l] + u] = in.hinit[l][u];
            if (p.cs[l]) p.cs[l][(size_t)s * p.Hp[l] + u] = in.cinit[l][u];
        }
    if (threadIdx.x == 0) p.events[s] = 0;
}

struct SesAdopt { const float* hs[SBR_MAX_LAYERS]; const float* cs[SBR_MAX_LAYERS]; const int* X; const int* len; int T, Bp, F; };
// row blockIdx.x of the batch -> slot slots[row]: every layer's state at the row's length (slot `len` of a_hs / a_cs = the state after
// len items), len events, and the ids of its last min(len, history) steps at the ring places those events have
__global__ void __launch_bounds__(256) ses_adopt_kernel(SesPool p, SesAdopt b, SesInit in, const int* __restrict__ slots) {
    const int r = blockIdx.x, s = slots[r];
    const int len = max(0, min(b.len[r], b.T));
    for (int l = 0; l < p.L; ++l) {
        const size_t src = ((size_t)len * b.Bp + r) * p.Hp[l], dst = ((size_t)(len & 1) * p.capacity + s) * p.Hp[l];
        for (int u = threadIdx.x; u < p.Hp[l]; u += 256) {      // (an empty row: the initial states themselves -- not every chain stores slot 0)
            p.hs[l][dst + u] = len ? b.hs[l][src + u] : in.hinit[l][u];
            if (p.cs[l]) p.cs[l][dst + u] = len ? b.cs[l][src + u] : in.cinit[l][u];
        }
    }
    for (int t = max(0, len - p.ring_len) + threadIdx.x; t < len; t += 256)
        p.ring[(size_t)s * p.ring_len + t % p.ring_len] = b.X[((size_t)r * b.T + t) * b.F];
    if (threadIdx.x == 0) p.events[s] = len;
}

// Parking (sbr_sessions_export / sbr_sessions_import): records [n][y.bytes] in a staging buffer <-> the slots
// slots[0 .. n).  `tps` threads (16 / 64 / 256, chosen on the host by the size of a record's state part) own one record, so a
// workgroup moves 256 / tps of them: a GRU-16 record (64 bytes of state) takes 16 threads, a two-layer LSTM-512 one (8 KB) the whole
// workgroup.  The state part moves in 16-byte pieces, thread t of a record the pieces t, t + tps, ... of every row, each byte read and
// written once (the records start on 16 bytes: the staging buffer does, y.bytes and y.head are multiples of 16, Hp is one of 16 floats).
// Both read the slot's event count where it decides the plane: pack from the pool, unpack from the record.
//
// pack: the record is CANONICAL -- id t of it is the id at ring place (events - kept + t) % ring_len, kept = min(events, ring_len),
// then -1 and zeros up to y.head; the states come from plane events & 1 of every layer.  It only reads the pool.
__global__ void __launch_bounds__(256) ses_pack_kernel(SesPool p, SesRecLayout y, const int* __restrict__ slots, int n, int tps,
                                                        unsigned char* __restrict__ out) {
    const int t = threadIdx.x % tps;
    const long long r = (long long)blockIdx.x * (256 / tps) + threadIdx.x / tps;
    if (r >= n) return;                                  // (no barrier in this kernel)
    const int s = slots[r];
    const long long ev = p.events[s];
    unsigned char* rec = out + (size_t)r * y.bytes;
    if (t == 0) *(long long*)rec = ev;
    const long long kept = min(ev, (long long)y.ring_len);
    const int* ring = p.ring + (size_t)s * y.ring_len;
    int* ids = (int*)(rec + 8);
    for (int i = t; i < (int)(y.head - 8) / 4; i += tps)
        ids[i] = i < kept ? ring[(int)((ev - kept + i) % y.ring_len)] : (i < y.ring_len ? -1 : 0);
    float* dst = (float*)(rec + y.head);
    for (int l = 0; l < y.L; ++l) {
        const int Hp = y.Hp[l];
        const size_t at = ((size_t)(ev & 1) * p.capacity + s) * Hp;
        for (int u = 4 * t; u < Hp; u += 4 * tps) *(f32x4*)(dst + u) = *(const f32x4*)(p.hs[l] + at + u);
        dst += Hp;
        if (!y.lstm) continue;
        for (int u = 4 * t; u < Hp; u += 4 * tps) *(f32x4*)(dst + u) = *(const f32x4*)(p.cs[l] + at + u);
        dst += Hp;
    }
}

// unpack, the inverse: the slot takes the record's event count, its states into plane events & 1 of every layer (the other plane is
// left alone: nothing reads it before a step writes it), and its WHOLE ring: place j holds id t of the record where
// (events - kept + t) % ring_len == j and t < kept, -1 otherwise -- nothing of the former occupant survives.  The slots of a call are
// distinct and every count and id was checked on the host.
__global__ void __launch_bounds__(256) ses_unpack_kernel(SesPool p, SesRecLayout y, const int* __restrict__ slots, int n, int tps,
                                                          const unsigned char* __restrict__ in) {
    const int t = threadIdx.x % tps;
    const long long r = (long long)blockIdx.x * (256 / tps) + threadIdx.x / tps;
    if (r >= n) return;
    const int s = slots[r];
    const unsigned char* rec = in + (size_t)r * y.bytes;
    const long long ev = *(const long long*)rec;
    if (t == 0) p.events[s] = ev;
    const long long kept = min(ev, (long long)y.ring_len);
    const int first = (int)((ev - kept) % y.ring_len);      // the ring place of the record's id 0
    const int* ids = (const int*)(rec + 8);
    int* ring = p.ring + (size_t)s * y.ring_len;
    for (int j = t; j < y.ring_len; j += tps) {
        const int i = (j - first + y.ring_len) % y.ring_len;
        ring[j] = i < kept ? ids[i] : -1;
    }
    const float* src = (const float*)(rec + y.head);
    for (int l = 0; l < y.L; ++l) {
        const int Hp = y.Hp[l];
        const size_t at = ((size_t)(ev & 1) * p.capacity + s) * Hp;
        for (int u = 4 * t; u < Hp; u += 4 * tps) *(f32x4*)(p.hs[l] + at + u) = *(const f32x4*)(src + u);
        src += Hp;
        if (!y.lstm) continue;
        for (int u = 4 * t; u < Hp; u += 4 * tps) *(f32x4*)(p.cs[l] + at + u) = *(const f32x4*)(src + u);
        src += Hp;
    }
}

__global__ void __launch_bounds__(256) ses_gather_top_kernel(SesPool p, const int* __restrict__ slots, float* __restrict__ out) {
    const int r = blockIdx.x, s = slots[r], l = p.L - 1, Hp = p.Hp[l];
    const float* src = p.hs[l] + ((size_t)(p.events[s] & 1) * p.capacity + s) * Hp;
    for (int u = threadIdx.x; u < Hp; u += 256) out[(size_t)r * Hp + u] = src[u];
}

// sbr_sessions_replay_ranks, before its first replay launch: row blockIdx.x of the call keeps its slot's event count and ring aside
// (the replay's own commit overwrites both)
__global__ void __launch_bounds__(64) ses_keep_kernel(SesPool p, const int* __restrict__ slots, long long* __restrict__ e0, int* __restrict__ ring) {
    const int r = blockIdx.x, s = slots[r];
    if (threadIdx.x == 0) e0[r] = p.events[s];
    if (ring)
        for (int t = threadIdx.x; t < p.ring_len; t += 64) ring[(size_t)r * p.ring_len + t] = p.ring[(size_t)s * p.ring_len + t];
}

template <int CELL>
hipError_t launch_step_cell(hipStream_t st, const SesStep& a, int in) {
    const dim3 grid((a.ly.Hp + 63) / 64, (a.n + 15) / 16);
    if (in == SES_IN_INDEX) ses_step_kernel<CELL, SES_IN_INDEX><<<grid, 256, 0, st>>>(a);
    else if (in == SES_IN_EMB) ses_step_kernel<CELL, SES_IN_EMB><<<grid, 256, 0, st>>>(a);
    else ses_step_kernel<CELL, SES_IN_DENSE><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}
hipError_t launch_ses_step(hipStream_t st, int cell, const SesStep& a, int in) {
    switch (cell) {
        case SBR_CELL_LSTM: return launch_step_cell<CELL_LSTM>(st, a, in);
        case SBR_CELL_GRU: return launch_step_cell<CELL_GRU>(st, a, in);
        default: return launch_step_cell<CELL_VANILLA>(st, a, in);
    }
}

template <int CELL>
hipError_t launch_replay_cell(hipStream_t st, const SesReplay& a, int in) {
    const unsigned grid = (unsigned)((a.n + 15) / 16);
    if (a.trace) {
        if (in == SES_IN_INDEX) ses_replay_kernel<CELL, SES_IN_INDEX, true><<<grid, 256, 0, st>>>(a);
        else ses_replay_kernel<CELL, SES_IN_EMB, true><<<grid, 256, 0, st>>>(a);
    } else if (in == SES_IN_INDEX) ses_replay_kernel<CELL, SES_IN_INDEX, false><<<grid, 256, 0, st>>>(a);
    else ses_replay_kernel<CELL, SES_IN_EMB, false><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}
hipError_t launch_ses_replay(hipStream_t st, int cell, const SesReplay& a, int in) {
    switch (cell) {
        case SBR_CELL_LSTM: return launch_replay_cell<CELL_LSTM>(st, a, in);
        case SBR_CELL_GRU: return launch_replay_cell<CELL_GRU>(st, a, in);
        default: return launch_replay_cell<CELL_VANILLA>(st, a, in);
    }
}

// layer l of the engine as the tile computation reads it
SesLayer ses_layer(const sbr_sessions* s, int l) {
    const sbr_handle* h = s->h;
    const Layout& y = h->lay;
    const LayerLayout& ly = y.layer[l];
    SesLayer a{};
    a.capacity = s->p.capacity;
    a.Hp = ly.Hp; a.K_in = ly.n_in_p;
    a.Whid = h->P(ly.p_Whid); a.Win = h->P(ly.p_Win); a.bias = h->P(ly.p_b); a.peep = h->P(ly.p_peep);
    a.hs = s->p.hs[l]; a.cs = s->p.cs[l];
    a.emb = y.E ? h->P(y.p_Emb) : nullptr; a.Ep = y.Ep;
    if (l > 0) { a.in_hs = s->p.hs[l - 1]; a.in_Hp = y.layer[l - 1].Hp; }
    a.relu = (y.cfg.cell == SBR_CELL_VANILLA && (l > 0 || y.E)) ? 1 : 0;      // stock RecurrentLayer: rectify (rec_shape, sbr_step.hip)
    return a;
}

void ses_free(sbr_sessions* s) {
    for (int l = 0; l < SBR_MAX_LAYERS; ++l) { if (s->p.hs[l]) (void)hipFree(s->p.hs[l]); if (s->p.cs[l]) (void)hipFree(s->p.cs[l]); }
    if (s->p.events) (void)hipFree(s->p.events);
    if (s->p.ring) (void)hipFree(s->p.ring);
    if (s->d_slots) (void)hipFree(s->d_slots);
    if (s->d_items) (void)hipFree(s->d_items);
    if (s->d_second) (void)hipFree(s->d_second);
    if (s->d_rows) (void)hipFree(s->d_rows);
    if (s->d_ev_items) (void)hipFree(s->d_ev_items);
    if (s->d_ev_second) (void)hipFree(s->d_ev_second);
    if (s->d_park) (void)hipFree(s->d_park);
    delete s;
}

template <class T>
int ses_alloc(T** p, size_t n, const char* what, const char* call = "sbr_sessions_create") {
    if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        sbr_set_error("%s: hipMalloc(%zu) of %s failed", call, n * sizeof(T), what);
        return SBR_ENOMEM;
    }
    return SBR_OK;
}

}  // namespace

static SesInit ses_init(const SesPool& p, const sbr_handle* h) {
    SesInit in{};
    for (int l = 0; l < p.L; ++l) { in.hinit[l] = h->P(h->lay.layer[l].p_hinit); in.cinit[l] = h->P(h->lay.layer[l].p_cinit); }
    return in;
}
hipError_t launch_ses_reset(hipStream_t st, const SesPool& p, const sbr_handle* h, const int* slots, long long n) {
    const SesInit in = ses_init(p, h);
    if (n <= 0) return hipSuccess;
    ses_reset_kernel<<<(unsigned)n, 256, 0, st>>>(p, in, slots);
    return hipGetLastError();
}
hipError_t launch_ses_gather_top(hipStream_t st, const SesPool& p, const int* slots, int rows, float* out) {
    if (rows <= 0) return hipSuccess;
    ses_gather_top_kernel<<<rows, 256, 0, st>>>(p, slots, out);
    return hipGetLastError();
}

hipError_t launch_ses_keep(hipStream_t st, const SesPool& p, const int* slots, long long n, long long* e0, int* ring) {
    if (n <= 0) return hipSuccess;
    ses_keep_kernel<<<(unsigned)n, 64, 0, st>>>(p, slots, e0, ring);
    return hipGetLastError();
}

// The record of a parked session for this engine and ring (include/sbr_rnn.h): pure host arithmetic
static SesRecLayout ses_record_layout(const Layout& y, int history) {
    SesRecLayout r{};
    r.L = y.L; r.ring_len = std::max(history, 1); r.lstm = y.cfg.cell == SBR_CELL_LSTM ? 1 : 0;
    r.head = (8 + (size_t)4 * r.ring_len + 15) / 16 * 16;
    r.bytes = r.head;
    for (int l = 0; l < y.L; ++l) { r.Hp[l] = y.layer[l].Hp; r.bytes += (size_t)r.Hp[l] * sizeof(float) * (r.lstm ? 2 : 1); }
    return r;
}
// FNV-1a, 64 bit, over the 32-bit little-endian words (record version 1, cell, L, Hp_0 .. Hp_{L-1}, ring_len)
static uint64_t ses_record_fingerprint(const SesRecLayout& r, int cell) {
    uint64_t f = 0xcbf29ce484222325ull;
    auto word = [&](uint32_t w) { for (int b = 0; b < 4; ++b) { f ^= (w >> (8 * b)) & 0xffu; f *= 0x100000001b3ull; } };
    word(1u); word((uint32_t)cell); word((uint32_t)r.L);
    for (int l = 0; l < r.L; ++l) word((uint32_t)r.Hp[l]);
    word((uint32_t)r.ring_len);
    return f;
}

// the calls keep out of a training step in flight: its side streams read and write the parameters (as the state calls do)
int sessions_state_check(const sbr_sessions* s, const char* call) {
    const sbr_handle* h = s->h;
    if (h->st.step_open || h->st.train_fwd_open) { sbr_set_error("%s: a training step is open (finish it with sbr_apply_update)", call); return SBR_ESTATE; }
    if (h->lag_pending >= 0) { sbr_set_error("%s: a lagged cost is pending (collect it with sbr_lagged_flush)", call); return SBR_ESTATE; }
    return SBR_OK;
}
// slots[0 .. n): inside the pool and (distinct) named once; found before anything is launched
int sessions_check_slots(sbr_sessions* s, const char* call, const int32_t* slots, long long n, bool distinct) {
    if (distinct && ++s->epoch == 0) { std::fill(s->stamp.begin(), s->stamp.end(), 0u); s->epoch = 1; }
    for (long long r = 0; r < n; ++r) {
        CHECK_ARG(slots[r] >= 0 && slots[r] < s->p.capacity, "%s: slots[%lld] = %d outside [0,%lld)", call, r, slots[r], s->p.capacity);
        if (!distinct) continue;
        CHECK_ARG(s->stamp[slots[r]] != s->epoch, "%s: slot %d is named twice (slots[%lld])", call, slots[r], r);
        s->stamp[slots[r]] = s->epoch;
    }
    return SBR_OK;
}

extern "C" int sbr_sessions_create(sbr_handle* h, int64_t capacity, int32_t history, sbr_sessions** out) {
    CHECK_ARG(h && out, "null argument");
    const Layout& y = h->lay;
    CHECK_ARG(y.D == 1, "sbr_sessions_create: a bidirectional engine has no state that has seen only the first p items");
    CHECK_ARG(capacity >= 1 && capacity <= 0x7fffffff, "sbr_sessions_create: capacity=%lld outside [1,2^31)", (long long)capacity);
    CHECK_ARG(history >= 0, "sbr_sessions_create: history=%d is negative", history);
    sbr_sessions* s = new (std::nothrow) sbr_sessions();
    if (!s) { sbr_set_error("sbr_sessions_create: out of host memory"); return SBR_ENOMEM; }
    s->h = h;
    s->p = SesPool{};
    s->p.capacity = capacity; s->p.L = y.L; s->p.history = history; s->p.ring_len = std::max(history, 1);
    s->d_slots = s->d_items = s->d_second = nullptr;
    s->d_rows = nullptr; s->d_ev_items = s->d_ev_second = nullptr; s->ev_cap = 0;
    s->epoch = 0;
    s->stamp.assign((size_t)capacity, 0u);
    s->rec = ses_record_layout(y, history); s->d_park = nullptr; s->park_cap = 0;
    int rc = SBR_OK;
    for (int l = 0; l < y.L && rc == SBR_OK; ++l) {
        s->p.Hp[l] = y.layer[l].Hp;
        rc = ses_alloc(&s->p.hs[l], (size_t)2 * capacity * y.layer[l].Hp, "the hidden states");
        if (rc == SBR_OK && y.cfg.cell == SBR_CELL_LSTM) rc = ses_alloc(&s->p.cs[l], (size_t)2 * capacity * y.layer[l].Hp, "the cell states");
    }
    if (rc == SBR_OK) rc = ses_alloc(&s->p.events, (size_t)capacity, "the event counts");
    if (rc == SBR_OK) rc = ses_alloc(&s->p.ring, (size_t)capacity * s->p.ring_len, "the history rings");
    if (rc == SBR_OK) rc = ses_alloc(&s->d_slots, (size_t)capacity, "the slot list");
    if (rc == SBR_OK) rc = ses_alloc(&s->d_items, (size_t)capacity, "the item list");
    if (rc == SBR_OK) rc = ses_alloc(&s->d_second, (size_t)capacity, "the second index list");
    if (rc != SBR_OK) { ses_free(s); return rc; }
    // every byte of the pool is defined from here on (the planes no reset writes, the rings), then every slot is reset
    hipError_t e = hipSuccess;
    for (int l = 0; l < y.L && e == hipSuccess; ++l) {
        e = hipMemsetAsync(s->p.hs[l], 0, (size_t)2 * capacity * s->p.Hp[l] * sizeof(float), h->stream);
        if (e == hipSuccess && s->p.cs[l]) e = hipMemsetAsync(s->p.cs[l], 0, (size_t)2 * capacity * s->p.Hp[l] * sizeof(float), h->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(s->p.ring, 0xFF, (size_t)capacity * s->p.ring_len * sizeof(int), h->stream);
    if (e == hipSuccess) e = launch_ses_reset(h->stream, s->p, h, nullptr, capacity);
    if (e != hipSuccess) { sbr_set_error("sbr_sessions_create: %s", hipGetErrorString(e)); ses_free(s); return SBR_EHIP; }
    *out = s;
    return SBR_OK;
}

extern "C" void sbr_sessions_destroy(sbr_sessions* s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->h->stream);      // launches in flight read and write the pool
    ses_free(s);
}

extern "C" int sbr_sessions_reset(sbr_sessions* s, const int32_t* slots, int64_t n) {
    CHECK_ARG(s, "null argument");
    sbr_handle* h = s->h;
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_reset")) != SBR_OK) return rc;
    if (!slots) { SBR_LAUNCH(launch_ses_reset(h->stream, s->p, h, nullptr, s->p.capacity)); return SBR_OK; }
    CHECK_ARG(n >= 0 && n <= s->p.capacity, "sbr_sessions_reset: n=%lld outside [0,capacity=%lld]", (long long)n, s->p.capacity);
    if ((rc = sessions_check_slots(s, "sbr_sessions_reset", slots, n, true)) != SBR_OK) return rc;
    if (n == 0) return SBR_OK;
    // (pageable host memory: the copy has left the caller's array when it returns)
    SBR_HIP(hipMemcpyAsync(s->d_slots, slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    SBR_LAUNCH(launch_ses_reset(h->stream, s->p, h, s->d_slots, n));
    return SBR_OK;
}

extern "C" int sbr_sessions_advance(sbr_sessions* s, const int32_t* slots, const int32_t* items, const int32_t* second, int64_t n) {
    CHECK_ARG(s && slots && items, "null argument");
    sbr_handle* h = s->h;
    const Layout& y = h->lay;
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_advance")) != SBR_OK) return rc;
    CHECK_ARG(n >= 0 && n <= s->p.capacity, "sbr_sessions_advance: n=%lld outside [0,capacity=%lld]", (long long)n, s->p.capacity);
    CHECK_ARG(y.F == 2 || !second, "sbr_sessions_advance: `second` given, but the model feeds one index per step");
    CHECK_ARG(y.F == 1 || second, "sbr_sessions_advance: the model feeds two indices per step: `second` is required");
    const int n_ids = y.cfg.input_size;
    for (int64_t r = 0; r < n; ++r) {
        CHECK_ARG(items[r] >= 0 && items[r] < n_ids, "sbr_sessions_advance: items[%lld] = %d outside [0,%d)", (long long)r, items[r], n_ids);
        if (second) CHECK_ARG(second[r] >= 0 && second[r] < n_ids, "sbr_sessions_advance: second[%lld] = %d outside [0,%d)", (long long)r, second[r], n_ids);
    }
    if ((rc = sessions_check_slots(s, "sbr_sessions_advance", slots, n, true)) != SBR_OK) return rc;
    if (n == 0) return SBR_OK;
    hipStream_t st = h->stream;
    // the rows of the index-addressed block that are read must be current (advance reads no output row)
    if ((rc = flush_lazy(h, 0)) != SBR_OK) return rc;
    // (pageable host memory: the copies have left the caller's arrays when they return)
    SBR_HIP(hipMemcpyAsync(s->d_slots, slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    SBR_HIP(hipMemcpyAsync(s->d_items, items, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    if (second) SBR_HIP(hipMemcpyAsync(s->d_second, second, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    for (int l = 0; l < y.L; ++l) {
        SesStep a{};
        a.n = (int)n; a.slots = s->d_slots; a.events = s->p.events;
        a.ly = ses_layer(s, l);
        a.items = s->d_items; a.second = second ? s->d_second : nullptr;
        SBR_LAUNCH(launch_ses_step(st, y.cfg.cell, a, l > 0 ? SES_IN_DENSE : (y.E ? SES_IN_EMB : SES_IN_INDEX)));
    }
    ses_commit_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(s->p, s->d_slots, s->d_items, (int)n);
    SBR_LAUNCH(hipGetLastError());
    return SBR_OK;
}

// Everything sbr_sessions_replay (and sbr_sessions_replay_ranks, `call`) refuses about its lists, before anything is launched
int ses_replay_check(sbr_sessions* s, const char* call, const int32_t* slots, int64_t n, const int32_t* items, const int32_t* second,
                     const int64_t* off) {
    const Layout& y = s->h->lay;
    int rc;
    CHECK_ARG(n >= 0 && n <= s->p.capacity, "%s: n=%lld outside [0,capacity=%lld]", call, (long long)n, s->p.capacity);
    CHECK_ARG(y.F == 2 || !second, "%s: `second` given, but the model feeds one index per step", call);
    CHECK_ARG(y.F == 1 || second || n == 0, "%s: the model feeds two indices per step: `second` is required", call);
    if (n == 0) return SBR_OK;
    CHECK_ARG(slots && off, "null argument");
    CHECK_ARG(off[0] == 0, "%s: off[0] = %lld, not 0", call, (long long)off[0]);
    for (int64_t r = 0; r < n; ++r)
        CHECK_ARG(off[r + 1] >= off[r], "%s: off[%lld] = %lld is below off[%lld] = %lld", call, (long long)(r + 1), (long long)off[r + 1],
                  (long long)r, (long long)off[r]);
    const int64_t total = off[n];
    CHECK_ARG(total == 0 || items, "null argument");
    if ((rc = sessions_check_slots(s, call, slots, n, true)) != SBR_OK) return rc;
    const int n_ids = y.cfg.input_size;
    for (int64_t r = 0; r < n; ++r)
        for (int64_t i = off[r]; i < off[r + 1]; ++i) {
            CHECK_ARG(items[i] >= 0 && items[i] < n_ids, "%s: items[%lld] = %d outside [0,%d) (event %lld of slot %d)", call, (long long)i,
                      items[i], n_ids, (long long)(i - off[r]), slots[r]);
            if (second) CHECK_ARG(second[i] >= 0 && second[i] < n_ids, "%s: second[%lld] = %d outside [0,%d) (event %lld of slot %d)", call,
                                  (long long)i, second[i], n_ids, (long long)(i - off[r]), slots[r]);
        }
    return SBR_OK;
}

// The device copy of a call's events: the pool's own buffers, grown when a call needs more and kept (hipFree waits for a replay still
// reading the old ones); then the index-input rows are made current (as in advance) and the events uploaded
int ses_replay_events(sbr_sessions* s, const char* call, const int32_t* items, const int32_t* second, int64_t total) {
    sbr_handle* h = s->h;
    int rc;
    if (total > s->ev_cap) {
        if (s->d_ev_items) (void)hipFree(s->d_ev_items);
        if (s->d_ev_second) (void)hipFree(s->d_ev_second);
        s->d_ev_items = s->d_ev_second = nullptr; s->ev_cap = 0;
        const int64_t cap = std::max<int64_t>(total, 1024);
        if ((rc = ses_alloc(&s->d_ev_items, (size_t)cap, "the event list", call)) != SBR_OK) return rc;
        if (h->lay.F == 2 && (rc = ses_alloc(&s->d_ev_second, (size_t)cap, "the second index list", call)) != SBR_OK) return rc;
        s->ev_cap = cap;
    }
    // the rows of the index-addressed block that are read must be current, as in advance
    if ((rc = flush_lazy(h, 0)) != SBR_OK) return rc;
    // (pageable host memory: the copies have left the host arrays when they return)
    SBR_HIP(hipMemcpyAsync(s->d_ev_items, items, (size_t)total * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (second) SBR_HIP(hipMemcpyAsync(s->d_ev_second, second, (size_t)total * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return SBR_OK;
}

// ONE launch over n_rows device rows (longest first): the events of every layer, the event counts and the rings (ses_replay_kernel's
// end is the commit); trace != NULL: the tracing form, trows beside rows
hipError_t launch_ses_replay_rows(sbr_sessions* s, const SesRow* d_rows, int n_rows, bool second, const SesTraceRow* trows, float* trace) {
    const Layout& y = s->h->lay;
    SesReplay a{};
    a.n = n_rows; a.L = y.L; a.rows = d_rows;
    a.items = s->d_ev_items; a.second = second ? s->d_ev_second : nullptr;
    a.events = s->p.events; a.ring = s->p.ring; a.ring_len = s->p.ring_len;
    for (int l = 0; l < y.L; ++l) a.ly[l] = ses_layer(s, l);
    a.trows = trows; a.trace = trace;
    return launch_ses_replay(s->h->stream, y.cfg.cell, a, y.E ? SES_IN_EMB : SES_IN_INDEX);
}

extern "C" int sbr_sessions_replay(sbr_sessions* s, const int32_t* slots, int64_t n, const int32_t* items, const int32_t* second,
                                   const int64_t* off) {
    CHECK_ARG(s, "null argument");
    sbr_handle* h = s->h;
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_replay")) != SBR_OK) return rc;
    h->last_replay_launches = 0;
    if ((rc = ses_replay_check(s, "sbr_sessions_replay", slots, n, items, second, off)) != SBR_OK) return rc;
    if (n == 0) return SBR_OK;
    const int64_t total = off[n];
    if (total == 0) return SBR_OK;
    // the rows that have events, longest first (stable): a tile's rows end together.  No output depends on which rows share a tile.
    std::vector<SesRow>& rows = s->rows;
    rows.clear();
    for (int64_t r = 0; r < n; ++r)
        if (off[r + 1] > off[r]) rows.push_back(SesRow{off[r], off[r + 1] - off[r], slots[r]});
    std::stable_sort(rows.begin(), rows.end(), [](const SesRow& a, const SesRow& b) { return a.len > b.len; });
    if (!s->d_rows && (rc = ses_alloc(&s->d_rows, (size_t)s->p.capacity, "the row list", "sbr_sessions_replay")) != SBR_OK) return rc;
    if ((rc = ses_replay_events(s, "sbr_sessions_replay", items, second, total)) != SBR_OK) return rc;
    SBR_HIP(hipMemcpyAsync(s->d_rows, rows.data(), rows.size() * sizeof(SesRow), hipMemcpyHostToDevice, h->stream));
    SBR_LAUNCH(launch_ses_replay_rows(s, s->d_rows, (int)rows.size(), second != nullptr, nullptr, nullptr));
    h->last_replay_launches = 1;
    return SBR_OK;
}

extern "C" int sbr_sessions_adopt(sbr_sessions* s, const int32_t* slots, int32_t n_rows) {
    CHECK_ARG(s && slots, "null argument");
    sbr_handle* h = s->h;
    const Layout& y = h->lay;
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_adopt")) != SBR_OK) return rc;
    if (!h->have_batch) { sbr_set_error("sbr_sessions_adopt: no batch set"); return SBR_ESTATE; }
    CHECK_ARG(n_rows >= 0 && n_rows <= h->n_rows, "sbr_sessions_adopt: n_rows=%d, the batch has %d rows", n_rows, h->n_rows);
    CHECK_ARG(n_rows <= s->p.capacity, "sbr_sessions_adopt: n_rows=%d above the capacity %lld", n_rows, s->p.capacity);
    if ((rc = sessions_check_slots(s, "sbr_sessions_adopt", slots, n_rows, true)) != SBR_OK) return rc;
    if (n_rows == 0) return SBR_OK;
    if ((rc = forward_current(h)) != SBR_OK) return rc;      // the chains' forward pass, if the batch has none yet
    SBR_HIP(hipMemcpyAsync(s->d_slots, slots, (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice, h->stream));
    SesAdopt b{};
    for (int l = 0; l < y.L; ++l) { b.hs[l] = h->A(y.layer[l].a_hs); b.cs[l] = h->A(y.layer[l].a_cs); }
    b.X = h->bX; b.len = h->blen; b.T = y.T; b.Bp = y.Bp; b.F = y.F;
    ses_adopt_kernel<<<n_rows, 256, 0, h->stream>>>(s->p, b, ses_init(s->p, h), s->d_slots);
    SBR_LAUNCH(hipGetLastError());
    return SBR_OK;
}

// where slot's current state of `layer` lies: its event count is read first (one wait)
static int ses_locate(sbr_sessions* s, const char* call, int32_t slot, int32_t layer, long long* events, size_t* at) {
    CHECK_ARG(slot >= 0 && slot < s->p.capacity, "%s: slot %d outside [0,%lld)", call, slot, s->p.capacity);
    CHECK_ARG(layer >= 0 && layer < s->p.L, "%s: layer %d outside [0,%d)", call, layer, s->p.L);
    hipStream_t st = s->h->stream;
    SBR_HIP(hipMemcpyAsync(events, s->p.events + slot, sizeof(long long), hipMemcpyDeviceToHost, st));
    SBR_HIP(hipStreamSynchronize(st));
    *at = ((size_t)(*events & 1) * s->p.capacity + slot) * s->p.Hp[layer];
    return SBR_OK;
}

extern "C" int sbr_sessions_read(sbr_sessions* s, int32_t slot, int32_t layer, float* h_host, float* c_host, int64_t* events, int32_t* history_host) {
    CHECK_ARG(s, "null argument");
    long long ev = 0; size_t at = 0;
    int rc;
    if ((rc = ses_locate(s, "sbr_sessions_read", slot, layer, &ev, &at)) != SBR_OK) return rc;
    hipStream_t st = s->h->stream;
    const size_t row = (size_t)s->p.Hp[layer] * sizeof(float);
    if (h_host) SBR_HIP(hipMemcpyAsync(h_host, s->p.hs[layer] + at, row, hipMemcpyDeviceToHost, st));
    if (c_host && s->p.cs[layer]) SBR_HIP(hipMemcpyAsync(c_host, s->p.cs[layer] + at, row, hipMemcpyDeviceToHost, st));
    std::vector<int> ring;
    if (history_host && s->p.history > 0) {
        ring.resize((size_t)s->p.ring_len);
        SBR_HIP(hipMemcpyAsync(ring.data(), s->p.ring + (size_t)slot * s->p.ring_len, ring.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    SBR_HIP(hipStreamSynchronize(st));
    if (history_host && s->p.history > 0) {
        const long long kept = std::min<long long>(ev, s->p.history);
        for (long long t = 0; t < s->p.history; ++t) history_host[t] = t < kept ? ring[(size_t)((ev - kept + t) % s->p.ring_len)] : -1;
    }
    if (events) *events = ev;
    return SBR_OK;
}

extern "C" int sbr_sessions_write(sbr_sessions* s, int32_t slot, int32_t layer, const float* h_host, const float* c_host) {
    CHECK_ARG(s && h_host, "null argument");
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_write")) != SBR_OK) return rc;
    CHECK_ARG(!s->p.cs[0] || c_host, "sbr_sessions_write: an LSTM layer's state is h and c: c_host is required");
    long long ev = 0; size_t at = 0;
    if ((rc = ses_locate(s, "sbr_sessions_write", slot, layer, &ev, &at)) != SBR_OK) return rc;
    hipStream_t st = s->h->stream;
    const size_t row = (size_t)s->p.Hp[layer] * sizeof(float);
    SBR_HIP(hipMemcpyAsync(s->p.hs[layer] + at, h_host, row, hipMemcpyHostToDevice, st));
    if (s->p.cs[layer]) SBR_HIP(hipMemcpyAsync(s->p.cs[layer] + at, c_host, row, hipMemcpyHostToDevice, st));
    SBR_HIP(hipStreamSynchronize(st));
    return SBR_OK;
}

// ---------------------------------------------------------------------------------------------------------------- parking
extern "C" int sbr_sessions_record_layout(const sbr_config* cfg, int32_t history, size_t* record_bytes, uint64_t* fingerprint) {
    CHECK_ARG(cfg && record_bytes && fingerprint, "null argument");
    Layout lay; std::string err;
    if (sbr_build_layout(*cfg, lay, err) != SBR_OK) { sbr_set_error("%s", err.c_str()); return SBR_EINVAL; }
    CHECK_ARG(lay.D == 1, "sbr_sessions_record_layout: a bidirectional engine has no state that has seen only the first p items");
    CHECK_ARG(history >= 0, "sbr_sessions_record_layout: history=%d is negative", history);
    const SesRecLayout r = ses_record_layout(lay, history);
    *record_bytes = r.bytes;
    *fingerprint = ses_record_fingerprint(r, lay.cfg.cell);
    return SBR_OK;
}

// The staging of one export / import: how many records a chunk holds, the buffer grown to hold them and their slot list (the old one
// is freed first, and hipFree waits for the device: replay's caveat), the threads per record.  Before anything is launched.
struct SesPark { int64_t chunk; size_t slots_at; int tps; };
static int ses_park_stage(sbr_sessions* s, const char* call, int64_t n, int64_t chunk_slots, SesPark* out) {
    const SesRecLayout& y = s->rec;
    int64_t chunk = chunk_slots > 0 ? chunk_slots : std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / y.bytes));
    chunk = std::min(chunk, n);
    const size_t slots_at = (size_t)chunk * y.bytes, need = slots_at + ((size_t)chunk * sizeof(int) + 15) / 16 * 16;
    if (need > s->park_cap) {
        if (s->d_park) (void)hipFree(s->d_park);
        s->d_park = nullptr; s->park_cap = 0;
        int rc;
        if ((rc = ses_alloc(&s->d_park, need, "the staging buffer", call)) != SBR_OK) return rc;
        s->park_cap = need;
    }
    const size_t pieces = (y.bytes - y.head) / 16;
    out->chunk = chunk; out->slots_at = slots_at;
    out->tps = pieces <= 32 ? 16 : (pieces <= 256 ? 64 : 256);
    return SBR_OK;
}

extern "C" int sbr_sessions_export(sbr_sessions* s, const int32_t* slots, int64_t n, int64_t chunk_slots, void* records_host, size_t cap) {
    CHECK_ARG(s, "null argument");
    sbr_handle* h = s->h;
    const SesRecLayout& y = s->rec;
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_export")) != SBR_OK) return rc;
    h->last_park_chunks = 0;
    CHECK_ARG(n >= 0 && n <= 0x7fffffff, "sbr_sessions_export: n=%lld outside [0,2^31)", (long long)n);
    CHECK_ARG(chunk_slots >= 0, "sbr_sessions_export: chunk_slots=%lld is negative", (long long)chunk_slots);
    if (n == 0) return SBR_OK;
    CHECK_ARG(slots && records_host, "null argument");
    CHECK_ARG(cap >= (size_t)n * y.bytes, "sbr_sessions_export: cap=%zu is below n * record_bytes = %lld * %zu = %zu", cap, (long long)n,
              y.bytes, (size_t)n * y.bytes);
    if ((rc = sessions_check_slots(s, "sbr_sessions_export", slots, n, false)) != SBR_OK) return rc;
    SesPark pk;
    if ((rc = ses_park_stage(s, "sbr_sessions_export", n, chunk_slots, &pk)) != SBR_OK) return rc;
    hipStream_t st = h->stream;
    int* d_slots = (int*)(s->d_park + pk.slots_at);
    int chunks = 0;
    for (int64_t r0 = 0; r0 < n; r0 += pk.chunk, ++chunks) {
        const int m = (int)std::min(pk.chunk, n - r0);
        // (the stream orders this chunk's kernel behind the copy that empties the buffer of the chunk before it)
        SBR_HIP(hipMemcpyAsync(d_slots, slots + r0, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
        const int per = 256 / pk.tps;
        ses_pack_kernel<<<(unsigned)((m + per - 1) / per), 256, 0, st>>>(s->p, y, d_slots, m, pk.tps, s->d_park);
        SBR_LAUNCH(hipGetLastError());
        SBR_HIP(hipMemcpyAsync((unsigned char*)records_host + (size_t)r0 * y.bytes, s->d_park, (size_t)m * y.bytes, hipMemcpyDeviceToHost, st));
    }
    SBR_HIP(hipStreamSynchronize(st));
    h->last_park_chunks = chunks;
    return SBR_OK;
}

extern "C" int sbr_sessions_import(sbr_sessions* s, const int32_t* slots, int64_t n, int64_t chunk_slots, const void* records_host, size_t bytes) {
    CHECK_ARG(s, "null argument");
    sbr_handle* h = s->h;
    const SesRecLayout& y = s->rec;
    int rc;
    if ((rc = sessions_state_check(s, "sbr_sessions_import")) != SBR_OK) return rc;
    h->last_park_chunks = 0;
    CHECK_ARG(n >= 0 && n <= s->p.capacity, "sbr_sessions_import: n=%lld outside [0,capacity=%lld]", (long long)n, s->p.capacity);
    CHECK_ARG(chunk_slots >= 0, "sbr_sessions_import: chunk_slots=%lld is negative", (long long)chunk_slots);
    CHECK_ARG(bytes == (size_t)n * y.bytes, "sbr_sessions_import: bytes=%zu is not n * record_bytes = %lld * %zu = %zu", bytes, (long long)n,
              y.bytes, (size_t)n * y.bytes);
    if (n == 0) return SBR_OK;
    CHECK_ARG(slots && records_host, "null argument");
    if ((rc = sessions_check_slots(s, "sbr_sessions_import", slots, n, true)) != SBR_OK) return rc;
    // every count and id, as advance would take them (the floats are not inspected, as write does not inspect them)
    const int n_ids = h->lay.cfg.input_size;
    std::vector<int>& ids = s->park_ids;
    ids.resize((size_t)y.ring_len);
    for (int64_t r = 0; r < n; ++r) {
        const unsigned char* rec = (const unsigned char*)records_host + (size_t)r * y.bytes;
        long long ev;
        memcpy(&ev, rec, sizeof(ev));
        memcpy(ids.data(), rec + 8, ids.size() * sizeof(int));
        CHECK_ARG(ev >= 0, "sbr_sessions_import: record %lld (slot %d): events = %lld is negative", (long long)r, slots[r], ev);
        const long long kept = std::min<long long>(ev, y.ring_len);
        for (int t = 0; t < y.ring_len; ++t) {
            if (t < kept)
                CHECK_ARG(ids[t] >= 0 && ids[t] < n_ids, "sbr_sessions_import: record %lld (slot %d): ids[%d] = %d outside [0,%d) among its %lld kept ids",
                          (long long)r, slots[r], t, ids[t], n_ids, kept);
            else
                CHECK_ARG(ids[t] == -1, "sbr_sessions_import: record %lld (slot %d): ids[%d] = %d behind its %lld kept ids, where only -1 may stand",
                          (long long)r, slots[r], t, ids[t], kept);
        }
    }
    SesPark pk;
    if ((rc = ses_park_stage(s, "sbr_sessions_import", n, chunk_slots, &pk)) != SBR_OK) return rc;
    hipStream_t st = h->stream;
    int* d_slots = (int*)(s->d_park + pk.slots_at);
    int chunks = 0;
    for (int64_t r0 = 0; r0 < n; r0 += pk.chunk, ++chunks) {
        const int m = (int)std::min(pk.chunk, n - r0);
        // (pageable host memory: the copies have left the caller's arrays when they return; the stream orders them behind the kernel
        // that reads the chunk before)
        SBR_HIP(hipMemcpyAsync(d_slots, slots + r0, (size_t)m * sizeof(int), hipMemcpyHostToDevice, st));
        SBR_HIP(hipMemcpyAsync(s->d_park, (const unsigned char*)records_host + (size_t)r0 * y.bytes, (size_t)m * y.bytes, hipMemcpyHostToDevice, st));
        const int per = 256 / pk.tps;
        ses_unpack_kernel<<<(unsigned)((m + per - 1) / per), 256, 0, st>>>(s->p, y, d_slots, m, pk.tps, s->d_park);
        SBR_LAUNCH(hipGetLastError());
    }
    h->last_park_chunks = chunks;
    return SBR_OK;
}
