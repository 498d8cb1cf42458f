// MPC on the learners' OWN models (mpg_model_mpc_cost_grad, mpg_model_mpc_solve, mpg_model_mpc_rollout; model_mpc.hip): the horizon cost of a control sequence
// on rollout::PathTracking / Pendulum / DoublePendulum (rollout_common.h), its gradient by the chain of ENV::vjp, and the problem type
// that mpc::solve (mpc_core.h) minimises it through - the one SPG loop of the project.  include/mpg_hip.h states the problem.
//
// The forward pass is the forward sweep's chain on the CARRIED state: s_{t+1}, rew_t = ENV::finish(ENV::pre(s_t, eps_t), u_t); the
// reverse pass is ENV::vjp from lam_H = 0 with rho = -1 (cost = -sum rew).  The model bodies are rollout_common.h's, untouched.
//
// One lane = one row, workgroups of one wave, as in mpc_core.h.  A lane's arrays are indexed by the running step and live in LDS as
// [index][lane] (64 lanes, 64 consecutive dwords, one per bank); nothing is addressed through a run-time-indexed private array:
//   U, G, T   ACT * H floats each (the solver; the cost kernel has U and G)
//   X         (H + 1) * OBS floats: the state BEFORE step i at X[(OBS * i + e) * WAVE], the state behind the last step at i = H -
//             ENV::vjp of step i reads states i and i + 1 (the pendulums take their reward on the NEW state)
//   E         H floats of model noise (not the double pendulum: its model has none)
//   ADJ       DoublePendulum::vjp works in ENV::ADJ = 24 CONTIGUOUS floats per lane: a block per lane at a stride of ADJ_STRIDE = 25
//             floats - odd, so that the 64 lanes' blocks start on 64 different banks (at 24 they would collide 8-way).
// H = 31: PathTracking 13 * 31 + 6 floats per lane = 102 272 bytes per workgroup for the solver, pendulum 8 * 31 + 4 = 64 512,
// double pendulum 9 * 31 + 6 + 25 = 79 360.
//
// No contraction, for mpc_core.h's reason: forward() is inlined into two kernels and a cost's bits must not depend on which
// (mpg_model_mpc_solve's cost_out is mpg_model_mpc_cost_grad's at the returned u).  The explicit fmaf calls of the model bodies stay
// fused in both.  Including units set the pragma BEFORE rollout_common.h, so that it covers the model bodies.
#pragma once
#include "mpc_core.h"
#include "rollout_common.h"

#pragma clang fp contract(off)

namespace model_mpc {

using mpc::WAVE;
using mpc::box;

constexpr int ADJ_STRIDE = 25;
template <class ENV> constexpr bool has_noise() { return !rollout::has_features<ENV>::value; }
template <class ENV> constexpr int adj_lds_floats() { return rollout::has_features<ENV>::value ? ADJ_STRIDE * WAVE : 0; }

// floats of LDS of one workgroup with n_ctrl control-sized arrays (2: the cost kernel's U, G; 3: the solver's U, G, T)
template <class ENV>
inline size_t lds_bytes(int H, int n_ctrl) {
    return ((size_t)(n_ctrl * ENV::ACT * H + (H + 1) * ENV::OBS + (has_noise<ENV>() ? H : 0)) * WAVE + adj_lds_floats<ENV>()) * sizeof(float);
}

// a lane's arrays behind the control-sized ones, carved from `p` (the first float behind them, lane 0)
template <class ENV>
struct Arrays {
    float *X, *E, *adj;
    __device__ __forceinline__ Arrays(float* p, int H, int lane) {
        X = p + lane;
        p += (H + 1) * ENV::OBS * WAVE;
        E = has_noise<ENV>() ? p + lane : nullptr;
        if (has_noise<ENV>()) p += H * WAVE;
        adj = rollout::has_features<ENV>::value ? p + lane * ADJ_STRIDE : nullptr;
    }
};

// s_0: the model's reading of a start row, as the sweeps take a START observation.  PathTracking: the six base entries, not wrapped,
// look-ahead entries not read; pendulum: the four entries; double pendulum: ENV::reset's atan2 of the row's sines and cosines.
// A lane behind the last row works on zeros (20 m/s straight ahead; upright at rest) and stores nothing.
struct Start {
    float s[8];
};
template <class ENV>
__device__ __forceinline__ Start load_start(const float* obs0, size_t row, int od, bool valid) {
    Start r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.s[k] = 0.f;
    if (valid) {
        const float* p = obs0 + row * od;
        if constexpr (rollout::has_features<ENV>::value) {
            ENV::reset(p, r.s);
        } else {
#pragma unroll
            for (int k = 0; k < ENV::OBS; ++k) r.s[k] = p[k];
        }
    }
    return r;
}

// cost = -sum_t rew_t (RAW rewards, t ascending) from s0 with the controls P[(ACT * i + k) * WAVE] and the noise E[i * WAVE].  Stores
// the states into X (above).  obs_row (nullable): this row's [H + 1][od] observations, rows 1 .. H written here in mpg_model_step's row
// format; rew_row (nullable): [H] raw rewards.
template <class ENV>
__device__ __forceinline__ float forward(int H, const Start& s0, const float* P, const float* E, float* X, float* obs_row, float* rew_row,
                                         int od) {
    constexpr int NS = ENV::OBS, ACT = ENV::ACT;
    float s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = s0.s[k];
    float cost = 0.f;
    for (int i = 0; i < H; ++i) {
        float* xs = X + NS * i * WAVE;
#pragma unroll
        for (int e = 0; e < NS; ++e) xs[e * WAVE] = s[e];
        float a[2] = {0.f, 0.f}, p[ENV::NPRE], on[8], rew;
#pragma unroll
        for (int k = 0; k < ACT; ++k) a[k] = P[(ACT * i + k) * WAVE];
        float eps = 0.f;
        if constexpr (has_noise<ENV>()) eps = E[i * WAVE];
        ENV::pre(s, eps, p);
        if constexpr (rollout::has_features<ENV>::value) {
            float tr[4];
            ENV::finish(p, a, on, rew, tr);
            if (obs_row) {
                float f[ENV::NFEAT];
                ENV::features(on, tr, f);
#pragma unroll
                for (int k = 0; k < ENV::NFEAT; ++k) obs_row[(i + 1) * ENV::NFEAT + k] = f[k];
            }
        } else {
            ENV::finish(p, a, on, rew);
            if (obs_row) {
                float* o = obs_row + (size_t)(i + 1) * od;
#pragma unroll
                for (int k = 0; k < NS; ++k) o[k] = on[k];
                for (int k = NS; k < od; ++k) o[k] = on[ENV::FUT_SRC];       // PathTracking's look-ahead entries: copies of delta_y
            }
        }
        if (rew_row) rew_row[i] = rew;
        cost -= rew;
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = on[k];
    }
    float* xs = X + NS * H * WAVE;
#pragma unroll
    for (int e = 0; e < NS; ++e) xs[e * WAVE] = s[e];
    return cost;
}

// The reverse pass over the states X of the last forward pass, taken at the point P: the chain of ENV::vjp from lam_H = 0 with
// rho = -1.  d cost / d (control j) goes to G[j * WAVE]; pg, ss, sy, U and UPDATE as mpc::reverse has them.  PathTracking's gate on the
// v_x clamp comes with its vjp; its x (entry 5) has no adjoint: lam[5] stays 0.
template <class ENV, bool UPDATE>
__device__ __forceinline__ void reverse(int H, const float* P, const float* X, float* adj, float* U, float* G, float& pg, float& ss,
                                        float& sy) {
    constexpr int NS = ENV::OBS, ACT = ENV::ACT;
    float lam[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) lam[k] = 0.f;
    pg = 0.f; ss = 0.f; sy = 0.f;
    auto commit = [&](int j, float gnew) {
        const float p = P[j * WAVE];
        if (UPDATE) {
            const float s = p - U[j * WAVE], y = gnew - G[j * WAVE];
            ss += s * s;
            sy += s * y;
            U[j * WAVE] = p;
        }
        G[j * WAVE] = gnew;
        const float v = fabsf(box(p - gnew) - p);
        pg = (pg != pg) ? pg : (!(v <= pg) ? v : pg);
    };
    for (int i = H - 1; i >= 0; --i) {
        const float* xs = X + NS * i * WAVE;
        float o[8], on[8], a[2] = {0.f, 0.f}, g[8], ga[2];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o[e] = e < NS ? xs[e * WAVE] : 0.f;
            on[e] = e < NS ? xs[(NS + e) * WAVE] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < ACT; ++k) a[k] = P[(ACT * i + k) * WAVE];
        if constexpr (rollout::has_features<ENV>::value) ENV::vjp(o, a, on, lam, -1.f, g, ga, adj);
        else ENV::vjp(o, a, on, lam, -1.f, g, ga);
#pragma unroll
        for (int k = ACT - 1; k >= 0; --k) commit(ACT * i + k, ga[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) lam[k] = g[k];
    }
}

// the problem mpc::solve minimises for this lane
template <class ENV>
struct Problem {
    int H;
    const Start& s0;
    Arrays<ENV> m;
    __device__ __forceinline__ int controls() const { return ENV::ACT * H; }
    __device__ __forceinline__ float forward(const float* P) const { return model_mpc::forward<ENV>(H, s0, P, m.E, m.X, nullptr, nullptr, 0); }
    template <bool UPDATE>
    __device__ __forceinline__ void reverse(const float* P, float* U, float* G, float& pg, float& ss, float& sy) const {
        model_mpc::reverse<ENV, UPDATE>(H, P, m.X, m.adj, U, G, pg, ss, sy);
    }
};

// ---- the closed loop (mpg_model_mpc_rollout): an observation row carried in registers from one step to the next ------------------------
// The entries of a row that the model reads: PathTracking's six base entries, the pendulum's four, the double pendulum's eight (the
// look-ahead entries and the double pendulum's 8 .. 10 never reach a model).
template <class ENV> constexpr int row_regs() { return rollout::has_features<ENV>::value ? 8 : ENV::OBS; }

// load_start's reading of a row held in registers: the same values from the same entries (an idle lane's row is zeros)
template <class ENV>
__device__ __forceinline__ Start start_of(const float (&o)[8]) {
    Start r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.s[k] = 0.f;
    if constexpr (rollout::has_features<ENV>::value) {
        ENV::reset(o, r.s);
    } else {
#pragma unroll
        for (int k = 0; k < ENV::OBS; ++k) r.s[k] = o[k];
    }
    return r;
}

// a row in mpg_model_step's format from its carried entries, as forward() writes rows 1 .. H of an observation record
template <class ENV>
__device__ __forceinline__ void store_row(float* dst, const float (&o)[8], int od) {
    constexpr int NR = row_regs<ENV>();
#pragma unroll
    for (int k = 0; k < NR; ++k) dst[k] = o[k];
    if constexpr (rollout::has_features<ENV>::value) {
#pragma unroll
        for (int k = NR; k < ENV::NFEAT; ++k) dst[k] = 0.f;
    } else {
        for (int k = NR; k < od; ++k) dst[k] = o[ENV::FUT_SRC];
    }
}

// The plant's step: forward() with ONE step from s0 with the action P[k * WAVE], k < ACT, under the noise eps - the one-step horizon
// cost, whose row 1 of the observation record is the new row `on` and whose raw reward is returned.  E[0], the planner's zero, holds
// eps for the step only.  The feature model's row comes out of forward() through a record in registers (the step count is the literal
// 1, so every index into it is a constant); the others' rows are the carried state itself, which forward() leaves behind its last
// step in X - the values it writes to a record.
template <class ENV>
__device__ __forceinline__ float plant_step(const Start& s0, const float* P, const Arrays<ENV>& m, float eps, float (&on)[8]) {
    float rew;
#pragma unroll
    for (int k = 0; k < 8; ++k) on[k] = 0.f;
    if constexpr (has_noise<ENV>()) m.E[0] = eps;
    if constexpr (rollout::has_features<ENV>::value) {
        float rec[2 * ENV::NFEAT];
        forward<ENV>(1, s0, P, m.E, m.X, rec, &rew, ENV::NFEAT);
#pragma unroll
        for (int k = 0; k < 8; ++k) on[k] = rec[ENV::NFEAT + k];
    } else {
        forward<ENV>(1, s0, P, m.E, m.X, nullptr, &rew, 0);
#pragma unroll
        for (int k = 0; k < ENV::OBS; ++k) on[k] = m.X[(ENV::OBS + k) * WAVE];
    }
    if constexpr (has_noise<ENV>()) m.E[0] = 0.f;
    return rew;
}

}  // namespace model_mpc
