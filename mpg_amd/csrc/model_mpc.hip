// MPC on the models the learners optimise through (rollout_common.h: PathTracking, Pendulum, DoublePendulum): the undiscounted horizon
// cost of a control sequence - the objective AMPC trains a policy on, minimised here exactly, one start row at a time -, its gradient by
// the chain of ENV::vjp, the batched box-constrained solve, and the receding-horizon closed loop of that solve and the model's step in
// one launch (mpg_model_mpc_rollout).  include/mpg_hip.h states the problem; the device code is model_mpc.h
// (forward, reverse, the problem type) and mpc_core.h (mpc::solve, the one SPG loop, with mpg_mpc_solve's constants MPG_MPC_SPG_M,
// MPG_MPC_SPG_HALVINGS, MPG_MPC_SPG_GAMMA, MPG_MPC_SPG_ALPHA0, MPG_MPC_SPG_ALPHA_MAX_STEP, MPG_MPC_SPG_ALPHA_LO, MPG_MPC_SPG_ALPHA_HI).
//
// The contraction rule stands BEFORE the model bodies are read: no contraction anywhere in this unit (model_mpc.h says why).
#pragma clang fp contract(off)
#include "model_mpc.h"
#include "env_internal.h"

namespace {
using namespace model_mpc;

// this row's observation record [H + 1][od]: row 0 is obs0 as given
__device__ __forceinline__ float* start_record(float* obs_traj, const float* obs0, size_t row, int H, int od) {
    float* rec = obs_traj + row * (size_t)(H + 1) * od;
    for (int k = 0; k < od; ++k) rec[k] = obs0[row * od + k];
    return rec;
}

template <class ENV>
__device__ __forceinline__ void load_noise(float* E, const float* eps, int H, int rows, int row, bool valid) {
    if constexpr (has_noise<ENV>())
        for (int i = 0; i < H; ++i) E[i * WAVE] = (eps && valid) ? eps[(size_t)i * rows + row] : 0.f;
}

template <class ENV>
__global__ void __launch_bounds__(WAVE) k_model_mpc_cost_grad(int rows, int H, int od, const float* __restrict__ obs0,
                                                              const float* __restrict__ u, const float* __restrict__ eps,
                                                              float* __restrict__ cost, float* __restrict__ grad,
                                                              float* __restrict__ obs_traj, float* __restrict__ rew_traj) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ACT = ENV::ACT;
    const int lane = threadIdx.x, row = blockIdx.x * WAVE + lane, n = ACT * H;
    const bool valid = row < rows;
    float* U = lds + lane;                      // [ACT H][WAVE]
    float* G = U + n * WAVE;                    // [ACT H][WAVE]
    const Arrays<ENV> m(lds + 2 * n * WAVE, H, lane);
    const Start s0 = load_start<ENV>(obs0, (size_t)row, od, valid);
    for (int j = 0; j < n; ++j) U[j * WAVE] = valid ? u[(size_t)row * n + j] : 0.f;
    load_noise<ENV>(m.E, eps, H, rows, row, valid);
    float* obs_row = (obs_traj && valid) ? start_record(obs_traj, obs0, (size_t)row, H, od) : nullptr;
    float* rew_row = (rew_traj && valid) ? rew_traj + (size_t)row * H : nullptr;
    const float f = forward<ENV>(H, s0, U, m.E, m.X, obs_row, rew_row, od);
    if (valid) cost[row] = f;
    if (grad) {                                 // (uniform)
        float pg, ss, sy;
        reverse<ENV, false>(H, U, m.X, m.adj, U, G, pg, ss, sy);
        if (valid)
            for (int j = 0; j < n; ++j) grad[(size_t)row * n + j] = G[j * WAVE];
    }
}

template <class ENV>
__global__ void __launch_bounds__(WAVE) k_model_mpc_solve(int rows, int H, int od, int iters, float tol, const float* __restrict__ obs0,
                                                          const float* __restrict__ eps, float* u_io, float* __restrict__ cost_out,
                                                          float* __restrict__ pgnorm_out, int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ACT = ENV::ACT;
    const int lane = threadIdx.x, row = blockIdx.x * WAVE + lane, n = ACT * H;
    const bool valid = row < rows;
    float* U = lds + lane;                      // the last accepted point [ACT H][WAVE]
    float* G = U + n * WAVE;                    // its gradient
    float* T = G + n * WAVE;                    // the trial point
    const Arrays<ENV> m(lds + 3 * n * WAVE, H, lane);
    const Start s0 = load_start<ENV>(obs0, (size_t)row, od, valid);
    for (int j = 0; j < n; ++j) U[j * WAVE] = valid ? box(u_io[(size_t)row * n + j]) : 0.f;
    load_noise<ENV>(m.E, eps, H, rows, row, valid);
    const mpc::Solved r = mpc::solve(Problem<ENV>{H, s0, m}, iters, tol, valid, U, G, T);
    if (valid) {
        for (int j = 0; j < n; ++j) u_io[(size_t)row * n + j] = U[j * WAVE];
        cost_out[row] = r.cost;
        pgnorm_out[row] = r.pgnorm;
        info[row] = r.info;
    }
}

// mpg_model_mpc_rollout.  `steps` times: record the row, solve from it at the noise means (mpc::solve on Problem<ENV>, the body of
// k_model_mpc_solve), record the plan, step the plant with the plan's first action under its own noise (plant_step: forward() with one
// step, the body of k_model_mpc_cost_grad at horizon 1).  One lane per agent, workgroups of one wave: the entries of the agent's row
// that the model reads stay in registers across the steps, the solver's arrays in dynamic LDS as in k_model_mpc_solve, E zeros.
// What the chain of launches hands on through global memory is handed on here in registers and LDS, the same float32 values:
//   the row: what forward() writes into row 1 of a record - the next start is load_start's reading of exactly those entries;
//   the start point: warm, the solution moved up by one action inside U (k_model_mpc_solve would clamp what it reads, which leaves
//     entries of the box, NaN and -0 included, as they are); cold, u_io again - the one array read after the prologue beside eps, and
//     one this kernel never writes in that mode.
// obs_io and (warm) u_io are written after the LAST step only; obs_traj[0] is copied from obs_io in the prologue, every later row of
// the record is stored from the registers when the step before it ends.  Every loop has a fixed bound and leaves early only on a
// wave-uniform condition; lanes behind the last agent work on zeros and store nothing.  k_mpc_rollout's notes (env_path_tracking.hip)
// hold here: the launch's pointers but u_io, the counts, the flag and the tolerance rest in LDS so that the solver's nested loops keep
// their scalar registers, and the copy loops stay rolled.
struct RolloutArgs {
    float *obs_io, *obs_traj, *plan_traj, *rew_traj, *cost_traj, *pgnorm_traj;
    const float* eps;
    int* info_traj;
    int n, od, warm;
    float tol;
};
template <class ENV>
__global__ void __launch_bounds__(WAVE) k_model_mpc_rollout(const RolloutArgs a, int steps, int H, int iters, float* u_io) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ RolloutArgs sArg;
    constexpr int ACT = ENV::ACT, NR = row_regs<ENV>();
    const int lane = threadIdx.x, i = blockIdx.x * WAVE + lane, n = ACT * H;
    const bool valid = i < a.n;
    if (lane == 0) sArg = a;                    // (one wave: LDS is in order within it)
    float* U = lds + lane;                      // the last accepted point [ACT H][WAVE]; between two solves the next one's start point
    float* G = U + n * WAVE;                    // its gradient
    float* T = G + n * WAVE;                    // the trial point
    const Arrays<ENV> m(lds + 3 * n * WAVE, H, lane);
    float o[8];                                 // the row's entries the model reads (an idle lane's: zeros)
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = 0.f;
    float* const start = u_io + (size_t)(valid ? i : 0) * n;      // this lane's row of u_io, kept as the lane's own pointer
    if (valid) {
        const int od = a.od;
        const float* p = a.obs_io + (size_t)i * od;
        float* ot = a.obs_traj + (size_t)i * od;
#pragma unroll
        for (int k = 0; k < NR; ++k) o[k] = p[k];
#pragma unroll 1
        for (int k = 0; k < od; ++k) ot[k] = p[k];                 // obs_traj[0]: the caller's row as given
    }
#pragma unroll 1
    for (int j = 0; j < n; ++j) U[j * WAVE] = valid ? box(start[j]) : 0.f;
    if constexpr (has_noise<ENV>()) {
#pragma unroll 1
        for (int j = 0; j < H; ++j) m.E[j * WAVE] = 0.f;           // the planner plans at the noise means
    }
    size_t row = (size_t)i;                     // t n + i
    __builtin_amdgcn_wave_barrier();
    const float tol = sArg.tol;
    for (int left = steps; left > 0; --left) {
        const Start s0 = start_of<ENV>(o);
        const mpc::Solved r = mpc::solve(Problem<ENV>{H, s0, m}, iters, tol, valid, U, G, T);
        float eps = 0.f;
        if (valid) {
            float* pt = sArg.plan_traj + row * n;
#pragma unroll 1
            for (int j = 0; j < n; ++j) pt[j] = U[j * WAVE];
            float* const ct = sArg.cost_traj;
            float* const gt = sArg.pgnorm_traj;
            int* const it = sArg.info_traj;
            if (ct) ct[row] = r.cost;
            if (gt) gt[row] = r.pgnorm;
            if (it) it[row] = r.info;
            if constexpr (has_noise<ENV>()) {
                const float* const e = sArg.eps;
                if (e) eps = e[row];
            }
        }
        float on[8];
        const float rew = plant_step<ENV>(s0, U, m, eps, on);     // (reads the plan's first action: before U moves)
        // the next solve's start point (behind the last step: what u_io takes, or nothing)
        if (__builtin_amdgcn_readfirstlane(sArg.warm)) {           // the plan one action later, its last action repeated
#pragma unroll 1
            for (int j = 0; j + ACT < n; ++j) U[j * WAVE] = U[(j + ACT) * WAVE];
        } else {                                                    // the caller's, which this launch never writes
#pragma unroll 1
            for (int j = 0; j < n; ++j) U[j * WAVE] = valid ? box(start[j]) : 0.f;
        }
        if (valid) {
            sArg.rew_traj[row] = rew;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = on[k];
        }
        row += (size_t)sArg.n;
        if (valid && left > 1) store_row<ENV>(sArg.obs_traj + row * sArg.od, o, sArg.od);
    }
    if (valid) {
        store_row<ENV>(sArg.obs_io + (size_t)i * sArg.od, o, sArg.od);
        if (sArg.warm) {
#pragma unroll 1
            for (int j = 0; j < n; ++j) start[j] = U[j * WAVE];
        }
    }
}

// launch(ENV{}) for the cfg's model
template <class Launch>
int with_model(const mpg_cfg_t* cfg, Launch&& launch) {
    if (cfg->env_kind == MPG_ENV_INVERTED_DOUBLE_PENDULUM) return launch(rollout::DoublePendulum{});
    if (cfg->env_kind == MPG_ENV_INVERTED_PENDULUM) return launch(rollout::Pendulum{});
    return launch(rollout::PathTracking{});
}

int max_iters_of(int env_kind) {
    return env_kind == MPG_ENV_INVERTED_DOUBLE_PENDULUM ? MPG_MODEL_MPC_MAX_ITERS_DOUBLE_PENDULUM
           : env_kind == MPG_ENV_INVERTED_PENDULUM      ? MPG_MODEL_MPC_MAX_ITERS_PENDULUM
                                                        : MPG_MODEL_MPC_MAX_ITERS_PATH_TRACKING;
}
static_assert(MPG_MODEL_MPC_MAX_ITERS_PATH_TRACKING <= MPG_MPC_MAX_ITERS && MPG_MODEL_MPC_MAX_ITERS_PENDULUM <= MPG_MPC_MAX_ITERS &&
                  MPG_MODEL_MPC_MAX_ITERS_DOUBLE_PENDULUM <= MPG_MPC_MAX_ITERS,
              "a per-kind cap is at most MPG_MPC_MAX_ITERS");

int max_rollout_work_of(int env_kind) {
    return env_kind == MPG_ENV_INVERTED_DOUBLE_PENDULUM ? MPG_MODEL_MPC_ROLLOUT_MAX_WORK_DOUBLE_PENDULUM
           : env_kind == MPG_ENV_INVERTED_PENDULUM      ? MPG_MODEL_MPC_ROLLOUT_MAX_WORK_PENDULUM
                                                        : MPG_MODEL_MPC_ROLLOUT_MAX_WORK_PATH_TRACKING;
}

}  // namespace

extern "C" int mpg_model_mpc_cost_grad(const mpg_cfg_t* cfg, int rows, int horizon, const float* obs0, const float* u, const float* eps,
                                       float* cost, float* grad, float* obs_traj, float* rew_traj, mpg_stream_t stream) {
    if (int rc = model_cfg_refusal("mpg_model_mpc_cost_grad", cfg)) return rc;
    MPG_REQUIRE(rows > 0, "mpg_model_mpc_cost_grad: no rows (rows %d)", rows);
    MPG_REQUIRE(horizon >= 1, "mpg_model_mpc_cost_grad: horizon >= 1 (got %d)", horizon);
    MPG_REQUIRE(horizon <= MPG_MPC_MAX_HORIZON, "mpg_model_mpc_cost_grad: horizon <= %d (got %d)", MPG_MPC_MAX_HORIZON, horizon);
    MPG_REQUIRE(obs0 && u && cost, "mpg_model_mpc_cost_grad: null pointer");
    if (int rc = tanh_range_refusal("mpg_model_mpc_cost_grad", cfg)) return rc;
    return with_model(cfg, [&](auto env) {
        typedef decltype(env) ENV;
        const size_t lds = lds_bytes<ENV>(horizon, 2);
        if (int rc = mpc::allow_lds("mpg_model_mpc_cost_grad", k_model_mpc_cost_grad<ENV>, lds)) return rc;
        hipLaunchKernelGGL(k_model_mpc_cost_grad<ENV>, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), lds, mpg_stream(stream), rows, horizon,
                           cfg->obs_dim, obs0, u, eps, cost, grad, obs_traj, rew_traj);
        MPG_CHECK_LAUNCH("mpg_model_mpc_cost_grad");
        return (int)MPG_OK;
    });
}

extern "C" int mpg_model_mpc_solve(const mpg_cfg_t* cfg, int rows, int horizon, int iters, float tol, const float* obs0, const float* eps,
                                   float* u_io, float* cost_out, float* pgnorm_out, int* info, mpg_stream_t stream) {
    if (int rc = model_cfg_refusal("mpg_model_mpc_solve", cfg)) return rc;
    MPG_REQUIRE(rows > 0, "mpg_model_mpc_solve: no rows (rows %d)", rows);
    MPG_REQUIRE(horizon >= 1, "mpg_model_mpc_solve: horizon >= 1 (got %d)", horizon);
    MPG_REQUIRE(horizon <= MPG_MPC_MAX_HORIZON, "mpg_model_mpc_solve: horizon <= %d (got %d)", MPG_MPC_MAX_HORIZON, horizon);
    MPG_REQUIRE(iters >= 0, "mpg_model_mpc_solve: iters >= 0 (got %d)", iters);
    // (what bounds one launch's run time on a shared device: the kind's measured cap, include/mpg_hip.h)
    MPG_REQUIRE(iters <= max_iters_of(cfg->env_kind), "mpg_model_mpc_solve: iters <= %d for env kind %d (got %d)",
                max_iters_of(cfg->env_kind), cfg->env_kind, iters);
    MPG_REQUIRE(tol >= 0.f, "mpg_model_mpc_solve: tol negative or NaN (%g)", (double)tol);
    MPG_REQUIRE(obs0 && u_io && cost_out && pgnorm_out && info, "mpg_model_mpc_solve: null pointer");
    if (int rc = tanh_range_refusal("mpg_model_mpc_solve", cfg)) return rc;
    return with_model(cfg, [&](auto env) {
        typedef decltype(env) ENV;
        const size_t lds = lds_bytes<ENV>(horizon, 3);
        if (int rc = mpc::allow_lds("mpg_model_mpc_solve", k_model_mpc_solve<ENV>, lds)) return rc;
        hipLaunchKernelGGL(k_model_mpc_solve<ENV>, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), lds, mpg_stream(stream), rows, horizon,
                           cfg->obs_dim, iters, tol, obs0, eps, u_io, cost_out, pgnorm_out, info);
        MPG_CHECK_LAUNCH("mpg_model_mpc_solve");
        return (int)MPG_OK;
    });
}

extern "C" int mpg_model_mpc_rollout(const mpg_cfg_t* cfg, int n, int steps, int horizon, int iters, float tol, int warm_start, float* obs_io,
                                     float* u_io, const float* eps, float* obs_traj, float* plan_traj, float* rew_traj, float* cost_traj,
                                     float* pgnorm_traj, int* info_traj, mpg_stream_t stream) {
    if (int rc = model_cfg_refusal("mpg_model_mpc_rollout", cfg)) return rc;
    MPG_REQUIRE(n > 0, "mpg_model_mpc_rollout: no agents (n %d)", n);
    MPG_REQUIRE(steps >= 1, "mpg_model_mpc_rollout: steps >= 1 (got %d)", steps);
    MPG_REQUIRE(steps <= MPG_MODEL_MPC_ROLLOUT_MAX_STEPS, "mpg_model_mpc_rollout: steps <= %d (got %d)", MPG_MODEL_MPC_ROLLOUT_MAX_STEPS, steps);
    MPG_REQUIRE(horizon >= 1, "mpg_model_mpc_rollout: horizon >= 1 (got %d)", horizon);
    MPG_REQUIRE(horizon <= MPG_MPC_MAX_HORIZON, "mpg_model_mpc_rollout: horizon <= %d (got %d)", MPG_MPC_MAX_HORIZON, horizon);
    MPG_REQUIRE(iters >= 0, "mpg_model_mpc_rollout: iters >= 0 (got %d)", iters);
    MPG_REQUIRE(iters <= max_iters_of(cfg->env_kind), "mpg_model_mpc_rollout: iters <= %d for env kind %d (got %d)",
                max_iters_of(cfg->env_kind), cfg->env_kind, iters);
    // (one launch's run time on a shared device: include/mpg_hip.h derives the bound; callers run longer loops in chunks)
    MPG_REQUIRE((long)steps * iters <= max_rollout_work_of(cfg->env_kind),
                "mpg_model_mpc_rollout: steps * iters = %ld solver iterations in one launch, at most %d for env kind %d", (long)steps * iters,
                max_rollout_work_of(cfg->env_kind), cfg->env_kind);
    MPG_REQUIRE(tol >= 0.f, "mpg_model_mpc_rollout: tol negative or NaN (%g)", (double)tol);
    MPG_REQUIRE(warm_start == 0 || warm_start == 1, "mpg_model_mpc_rollout: warm_start is 0 or 1 (got %d)", warm_start);
    MPG_REQUIRE(obs_io && u_io && obs_traj && plan_traj && rew_traj, "mpg_model_mpc_rollout: null pointer");
    if (int rc = tanh_range_refusal("mpg_model_mpc_rollout", cfg)) return rc;
    return with_model(cfg, [&](auto env) {
        typedef decltype(env) ENV;
        const size_t lds = lds_bytes<ENV>(horizon, 3);
        if (int rc = mpc::allow_lds("mpg_model_mpc_rollout", k_model_mpc_rollout<ENV>, lds)) return rc;
        const RolloutArgs a = {obs_io, obs_traj, plan_traj, rew_traj, cost_traj, pgnorm_traj, eps, info_traj, n, cfg->obs_dim, warm_start, tol};
        hipLaunchKernelGGL(k_model_mpc_rollout<ENV>, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), lds, mpg_stream(stream), a, steps, horizon, iters,
                           u_io);
        MPG_CHECK_LAUNCH("mpg_model_mpc_rollout");
        return (int)MPG_OK;
    });
}
