// Evaluator.metrics_for_an_episode (evaluator.py:160-211) for every episode of a recorded evaluation, and the mean of each metric over
// the episodes (evaluator.py:153-156), in ONE launch: what the evaluator otherwise forms with about twenty torch launches and one
// synchronising .item() per metric comes back as one array of K * (n + 1) doubles.
//
// The trajectories are the ones mpg_eval_rollout / mpg_eval_rollout_pendulum record (or torch.stack of the per-step tensors):
// obs_traj [steps][n][obs_dim], act_traj [steps][n][act_dim], rew_traj [steps][n], float32.  Every entry is widened to double first and
// all arithmetic is double (the reference accumulates in numpy / python floats), products and sums rounded separately as numpy rounds
// them (no contraction).  This is not a hot loop: one lane per episode runs its sums over t ascending, a workgroup barrier, then lane k
// sums row k over the episodes ascending - fixed orders, no atomics, so two launches give the same bits.  One workgroup: an evaluation
// has tens of episodes (the parsers' num_eval_agent is 1, 5 or 50); more than 256 are served in rounds.
#include "mpg_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int STATIONARY_FROM = 20;      // evaluator.py:173, rew_list[20:]
constexpr int MSE_WINDOW = 25;           // evaluator.py:198-201, [:25]

// PathTracking-v0, evaluator.py:165-183.  Rows: episode_return, episode_len, delta_y_mse (obs column 3), delta_phi_mse (4), delta_v_mse
// (0), stationary_rew_mean, steer_mse, acc_mse.
__device__ __forceinline__ void path_tracking_episode(int n, int steps, int od, int i, const float* __restrict__ obs,
                                                      const float* __restrict__ act, const float* __restrict__ rew,
                                                      double* __restrict__ pe) {
    double ret = 0., sy = 0., sphi = 0., sv = 0., stat = 0., ssteer = 0., sacc = 0.;
    for (int t = 0; t < steps; ++t) {
        const size_t row = (size_t)t * n + i;
        const float* o = obs + row * od;
        const double r = (double)rew[row], dv = (double)o[0], dy = (double)o[3], dphi = (double)o[4];
        // :169-170, operator by operator: x[0] * 1.2 * np.pi / 9 and x[1] * 3.
        const double steer = (double)act[row * 2] * 1.2 * 3.141592653589793 / 9., acc = (double)act[row * 2 + 1] * 3.;
        ret += r;
        if (t >= STATIONARY_FROM) stat += r;
        sy += dy * dy;
        sphi += dphi * dphi;
        sv += dv * dv;
        ssteer += steer * steer;
        sacc += acc * acc;
    }
    const double len = (double)steps, tail = (double)(steps > STATIONARY_FROM ? steps - STATIONARY_FROM : 0);
    pe[0 * (size_t)n + i] = ret;
    pe[1 * (size_t)n + i] = len;
    pe[2 * (size_t)n + i] = sqrt(sy / len);
    pe[3 * (size_t)n + i] = sqrt(sphi / len);
    pe[4 * (size_t)n + i] = sqrt(sv / len);
    pe[5 * (size_t)n + i] = stat / tail;          // no step from 20 on: 0 / 0 = NaN, the mean of an empty list
    pe[6 * (size_t)n + i] = sqrt(ssteer / len);
    pe[7 * (size_t)n + i] = sqrt(sacc / len);
}

// InvertedPendulumConti-v0, evaluator.py:184-209.  Rows: episode_return, episode_len, then (mean, var) of x, theta, xdot, thetadot, the
// four root mean squares, and the four over the first 25 steps.  np.var: the population variance about the mean, in a second pass.
__device__ __forceinline__ void pendulum_episode(int n, int steps, int i, const float* __restrict__ obs, const float* __restrict__ rew,
                                                 double* __restrict__ pe) {
    const float4* o4 = reinterpret_cast<const float4*>(obs);
    const int win = steps < MSE_WINDOW ? steps : MSE_WINDOW;
    double ret = 0.;
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0., q0 = 0., q1 = 0., q2 = 0., q3 = 0., w0 = 0., w1 = 0., w2 = 0., w3 = 0.;
    for (int t = 0; t < steps; ++t) {
        const size_t row = (size_t)t * n + i;
        const float4 o = o4[row];
        const double x0 = (double)o.x, x1 = (double)o.y, x2 = (double)o.z, x3 = (double)o.w;
        ret += (double)rew[row];
        s0 += x0; s1 += x1; s2 += x2; s3 += x3;
        q0 += x0 * x0; q1 += x1 * x1; q2 += x2 * x2; q3 += x3 * x3;
        if (t < win) { w0 += x0 * x0; w1 += x1 * x1; w2 += x2 * x2; w3 += x3 * x3; }
    }
    const double len = (double)steps, wl = (double)win;
    const double m0 = s0 / len, m1 = s1 / len, m2 = s2 / len, m3 = s3 / len;
    double v0 = 0., v1 = 0., v2 = 0., v3 = 0.;
    for (int t = 0; t < steps; ++t) {
        const float4 o = o4[(size_t)t * n + i];
        const double d0 = (double)o.x - m0, d1 = (double)o.y - m1, d2 = (double)o.z - m2, d3 = (double)o.w - m3;
        v0 += d0 * d0; v1 += d1 * d1; v2 += d2 * d2; v3 += d3 * d3;
    }
    const size_t N = (size_t)n;
    pe[0 * N + i] = ret;
    pe[1 * N + i] = len;
    pe[2 * N + i] = m0; pe[3 * N + i] = v0 / len;
    pe[4 * N + i] = m1; pe[5 * N + i] = v1 / len;
    pe[6 * N + i] = m2; pe[7 * N + i] = v2 / len;
    pe[8 * N + i] = m3; pe[9 * N + i] = v3 / len;
    pe[10 * N + i] = sqrt(q0 / len); pe[11 * N + i] = sqrt(q1 / len); pe[12 * N + i] = sqrt(q2 / len); pe[13 * N + i] = sqrt(q3 / len);
    pe[14 * N + i] = sqrt(w0 / wl); pe[15 * N + i] = sqrt(w1 / wl); pe[16 * N + i] = sqrt(w2 / wl); pe[17 * N + i] = sqrt(w3 / wl);
}

template <int KIND>
__global__ void __launch_bounds__(NT) k_eval_metrics(int n, int steps, int od, const float* __restrict__ obs, const float* __restrict__ act,
                                                     const float* __restrict__ rew, double* pe, double* __restrict__ mean) {
    constexpr int K = KIND == MPG_ENV_PATH_TRACKING ? MPG_EVAL_METRICS_PATH_TRACKING : MPG_EVAL_METRICS_PENDULUM;
    static_assert(K <= NT, "one lane per metric forms the means");
    for (int i = threadIdx.x; i < n; i += NT) {
        if constexpr (KIND == MPG_ENV_PATH_TRACKING) path_tracking_episode(n, steps, od, i, obs, act, rew, pe);
        else pendulum_episode(n, steps, i, obs, rew, pe);
    }
    __threadfence_block();
    __syncthreads();                     // every per-episode row is written (by this workgroup) before it is summed
    if (threadIdx.x < K) {
        const double* row = pe + (size_t)threadIdx.x * n;
        double s = 0.;
        for (int i = 0; i < n; ++i) s += row[i];
        mean[threadIdx.x] = s / (double)n;
    }
}

}  // namespace

extern "C" int mpg_eval_metrics(int env_kind, int n, int steps, int obs_dim, const float* obs_traj, const float* act_traj,
                                const float* rew_traj, double* per_episode, double* mean, mpg_stream_t stream) {
    MPG_REQUIRE(env_kind == MPG_ENV_PATH_TRACKING || env_kind == MPG_ENV_INVERTED_PENDULUM,
                "mpg_eval_metrics: env kind %d has no evaluation metrics (PathTracking 0, the pendulum 1)", env_kind);
    MPG_REQUIRE(n > 0, "mpg_eval_metrics: no episodes (n %d)", n);
    MPG_REQUIRE(steps >= 1, "mpg_eval_metrics: steps >= 1 (got %d)", steps);
    if (env_kind == MPG_ENV_PATH_TRACKING)
        MPG_REQUIRE(obs_dim >= 6 && obs_dim <= 6 + MPG_ENV_MAX_FUTURE, "mpg_eval_metrics: obs_dim 6 .. 16 on PathTracking (got %d)", obs_dim);
    else
        MPG_REQUIRE(obs_dim == 4, "mpg_eval_metrics: obs_dim 4 on the pendulum (got %d)", obs_dim);
    MPG_REQUIRE(obs_traj && act_traj && rew_traj && per_episode && mean, "mpg_eval_metrics: null pointer");
    hipStream_t s = mpg_stream(stream);
    if (env_kind == MPG_ENV_PATH_TRACKING)
        hipLaunchKernelGGL(k_eval_metrics<MPG_ENV_PATH_TRACKING>, dim3(1), dim3(NT), 0, s, n, steps, obs_dim, obs_traj, act_traj, rew_traj,
                           per_episode, mean);
    else
        hipLaunchKernelGGL(k_eval_metrics<MPG_ENV_INVERTED_PENDULUM>, dim3(1), dim3(NT), 0, s, n, steps, obs_dim, obs_traj, act_traj, rew_traj,
                           per_episode, mean);
    MPG_CHECK_LAUNCH("mpg_eval_metrics");
    return MPG_OK;
}
