// The MPC baseline of the reference, SLSQP form (mpc/main.py): the horizon cost ModelPredictiveControl.cost_function (:156-165), its
// gradient by a hand adjoint, and a batched box-constrained minimiser - spectral projected gradient (Birgin, Martinez, Raydan 2000) -
// that runs a whole solve for every row in ONE launch.  include/mpg_hip.h states the problem, the method and its constants; the device
// code - forward, reverse and the solve, one lane per row with its arrays in LDS - is mpc_core.h, which mpg_mpc_rollout
// (env_path_tracking.hip) shares.  The method's constants as that code names them: MPG_MPC_STEER_SCALE and MPG_MPC_ACC_SCALE in both
// passes; MPG_MPC_SPG_M, MPG_MPC_SPG_HALVINGS, MPG_MPC_SPG_GAMMA, MPG_MPC_SPG_ALPHA0, MPG_MPC_SPG_ALPHA_MAX_STEP, MPG_MPC_SPG_ALPHA_LO
// and MPG_MPC_SPG_ALPHA_HI in the solve.
#include "mpc_core.h"

#pragma clang fp contract(off)

namespace {
using namespace mpc;

__device__ __forceinline__ State load_state(const float* x0, int row, bool valid) {
    State s = idle_state();
    if (valid) {
        const float* p = x0 + (size_t)row * 6;
        s.vx = p[0]; s.vy = p[1]; s.r = p[2]; s.dy = p[3]; s.dphi = p[4]; s.x = p[5];
    }
    return s;
}

__global__ void __launch_bounds__(WAVE) k_mpc_cost_grad(int rows, int H, const float* __restrict__ x0, const float* __restrict__ u,
                                                        float* __restrict__ cost, float* __restrict__ grad, float* __restrict__ traj) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, row = blockIdx.x * WAVE + lane;
    const bool valid = row < rows;
    float* U = lds + lane;                      // [2 H][WAVE]
    float* G = U + 2 * H * WAVE;                // [2 H][WAVE]
    float* X = G + 2 * H * WAVE;                // [NX H][WAVE]
    const State s0 = load_state(x0, row, valid);
    for (int j = 0; j < 2 * H; ++j) U[j * WAVE] = valid ? u[(size_t)row * 2 * H + j] : 0.f;
    const float f = forward(H, s0, U, X, (traj && valid) ? traj + (size_t)row * (H + 1) * 6 : nullptr);
    if (valid) cost[row] = f;
    if (grad) {                                 // (uniform)
        float pg, ss, sy;
        reverse<false>(H, U, X, U, G, pg, ss, sy);
        if (valid)
            for (int j = 0; j < 2 * H; ++j) grad[(size_t)row * 2 * H + j] = G[j * WAVE];
    }
}

__global__ void __launch_bounds__(WAVE) k_mpc_solve(int rows, int H, int iters, float tol, const float* __restrict__ x0, float* u_io,
                                                    float* __restrict__ cost_out, float* __restrict__ pgnorm_out, int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, row = blockIdx.x * WAVE + lane;
    const bool valid = row < rows;
    float* U = lds + lane;                      // the last accepted point [2 H][WAVE]
    float* G = U + 2 * H * WAVE;                // its gradient
    float* T = G + 2 * H * WAVE;                // the trial point
    float* X = T + 2 * H * WAVE;                // the states of the last forward pass [NX H][WAVE]
    const State s0 = load_state(x0, row, valid);
    for (int j = 0; j < 2 * H; ++j) U[j * WAVE] = valid ? box(u_io[(size_t)row * 2 * H + j]) : 0.f;
    const Solved r = solve(H, iters, tol, valid, s0, U, G, T, X);
    if (valid) {
        for (int j = 0; j < 2 * H; ++j) u_io[(size_t)row * 2 * H + j] = U[j * WAVE];
        cost_out[row] = r.cost;
        pgnorm_out[row] = r.pgnorm;
        info[row] = r.info;
    }
}

}  // namespace

extern "C" int mpg_mpc_cost_grad(int rows, int horizon, const float* x0, const float* u, float* cost, float* grad, float* traj,
                                 mpg_stream_t stream) {
    MPG_REQUIRE(rows > 0, "mpg_mpc_cost_grad: no rows (rows %d)", rows);
    MPG_REQUIRE(horizon >= 1, "mpg_mpc_cost_grad: horizon >= 1 (got %d)", horizon);
    MPG_REQUIRE(horizon <= MPG_MPC_MAX_HORIZON, "mpg_mpc_cost_grad: horizon <= %d (got %d)", MPG_MPC_MAX_HORIZON, horizon);
    MPG_REQUIRE(x0 && u && cost, "mpg_mpc_cost_grad: null pointer");
    const size_t lds = lds_bytes(horizon, 2);
    if (int rc = allow_lds("mpg_mpc_cost_grad", k_mpc_cost_grad, lds)) return rc;
    hipLaunchKernelGGL(k_mpc_cost_grad, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), lds, mpg_stream(stream), rows, horizon, x0, u, cost,
                       grad, traj);
    MPG_CHECK_LAUNCH("mpg_mpc_cost_grad");
    return MPG_OK;
}

extern "C" int mpg_mpc_solve(int rows, int horizon, int iters, float tol, const float* x0, float* u_io, float* cost_out, float* pgnorm_out,
                             int* info, mpg_stream_t stream) {
    MPG_REQUIRE(rows > 0, "mpg_mpc_solve: no rows (rows %d)", rows);
    MPG_REQUIRE(horizon >= 1, "mpg_mpc_solve: horizon >= 1 (got %d)", horizon);
    MPG_REQUIRE(horizon <= MPG_MPC_MAX_HORIZON, "mpg_mpc_solve: horizon <= %d (got %d)", MPG_MPC_MAX_HORIZON, horizon);
    MPG_REQUIRE(iters >= 0, "mpg_mpc_solve: iters >= 0 (got %d)", iters);
    MPG_REQUIRE(iters <= MPG_MPC_MAX_ITERS, "mpg_mpc_solve: iters <= %d (got %d)", MPG_MPC_MAX_ITERS, iters);
    MPG_REQUIRE(tol >= 0.f, "mpg_mpc_solve: tol negative or NaN (%g)", (double)tol);
    MPG_REQUIRE(x0 && u_io && cost_out && pgnorm_out && info, "mpg_mpc_solve: null pointer");
    const size_t lds = lds_bytes(horizon, 3);
    if (int rc = allow_lds("mpg_mpc_solve", k_mpc_solve, lds)) return rc;
    hipLaunchKernelGGL(k_mpc_solve, dim3((rows + WAVE - 1) / WAVE), dim3(WAVE), lds, mpg_stream(stream), rows, horizon, iters, tol, x0, u_io,
                       cost_out, pgnorm_out, info);
    MPG_CHECK_LAUNCH("mpg_mpc_solve");
    return MPG_OK;
}
