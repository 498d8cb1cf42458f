// Internal interface between the env entry points (env_path_tracking.hip) and the second real environment.
#pragma once
#include "mpg_common.h"

// the replay ring's five arrays, as the step -> ring -> reset kernels of both environments take them
struct RingPtrs {
    float *obs, *act, *rew, *obs2;
    uint8_t* done;
};

// a 64-bit Philox key and a 64-bit counter as the kernels' four 32-bit arguments (k0, k1, c1, c2)
#define MPG_KEY_CTR(key, ctr) (uint32_t)(key), (uint32_t)((key) >> 32), (uint32_t)(ctr), (uint32_t)((ctr) >> 32)

// MPG_ENV_INVERTED_DOUBLE_PENDULUM names a differentiable model only (include/mpg_hip.h): every real-env entry point refuses it
#define MPG_NO_DOUBLE_PENDULUM_ENV \
    "the real InvertedDoublePendulum-v2 env is MuJoCo and is not provided (only its differentiable model is: the rollout entry points)"

// ---- The refusals the one-launch rollouts of both environments share, stated once the way gauss::gauss_refusal is (gauss_head.h):
// `entry` names the caller in every text, MPG_OK lets the call proceed.  What an entry point alone asks stays in its body.

// what a launch built for one real env asks of a cfg, and the words its refusals say it in
struct EnvDesc {
    int kind, obs_lo, obs_hi, act_dim;
    const char *name, *obs_dims;
};
constexpr EnvDesc PATH_TRACKING_ENV{MPG_ENV_PATH_TRACKING, 6, 6 + MPG_ENV_MAX_FUTURE, 2, "path-tracking", "6 .. 16"};
constexpr EnvDesc PENDULUM_ENV{MPG_ENV_INVERTED_PENDULUM, 4, 4, 1, "pendulum", "4"};

// a cfg of env `e`: not null, not the double pendulum, no other env kind (each env has a launch of its own: mpg_*_rollout[_pendulum])
inline int env_kind_refusal(const char* entry, const EnvDesc& e, const mpg_cfg_t* cfg) {
    MPG_REQUIRE(cfg, "%s: null configuration", entry);
    MPG_REQUIRE(cfg->env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "%s: " MPG_NO_DOUBLE_PENDULUM_ENV, entry);
    MPG_REQUIRE(cfg->env_kind == e.kind, "%s: %s env only (env kind %d)", entry, e.name, cfg->env_kind);
    return MPG_OK;
}

// ... and of its widths (mpg_worker_sample_rollout_pendulum leaves them to gauss::squash_refusal, whose texts its callers know)
inline int env_cfg_refusal(const char* entry, const EnvDesc& e, const mpg_cfg_t* cfg) {
    if (int rc = env_kind_refusal(entry, e, cfg)) return rc;
    MPG_REQUIRE(cfg->obs_dim >= e.obs_lo && cfg->obs_dim <= e.obs_hi, "%s: obs_dim %s only (got %d)", entry, e.obs_dims, cfg->obs_dim);
    MPG_REQUIRE(cfg->act_dim == e.act_dim, "%s: act_dim %d only (got %d)", entry, e.act_dim, cfg->act_dim);
    return MPG_OK;
}

// what the entry points on the differentiable MODELS (model_rollout.hip) ask of a cfg: one of the three models - the double pendulum
// is served there - with that model's widths
inline int model_cfg_refusal(const char* entry, const mpg_cfg_t* cfg) {
    constexpr EnvDesc MODELS[] = {PATH_TRACKING_ENV, PENDULUM_ENV, {MPG_ENV_INVERTED_DOUBLE_PENDULUM, 11, 11, 1, "double-pendulum", "11"}};
    MPG_REQUIRE(cfg, "%s: null configuration", entry);
    const EnvDesc* m = nullptr;
    for (const EnvDesc& d : MODELS)
        if (d.kind == cfg->env_kind) m = &d;
    MPG_REQUIRE(m, "%s: unknown env kind %d (the models: 0 path tracking, 1 pendulum, 2 double pendulum)", entry, cfg->env_kind);
    MPG_REQUIRE(cfg->obs_dim >= m->obs_lo && cfg->obs_dim <= m->obs_hi, "%s: the %s model has obs_dim %s (got %d)", entry, m->name,
                m->obs_dims, cfg->obs_dim);
    MPG_REQUIRE(cfg->act_dim == m->act_dim, "%s: the %s model has act_dim %d (got %d)", entry, m->name, m->act_dim, cfg->act_dim);
    return MPG_OK;
}

// (the same refusal as net_cfg_ok, host_glue.h: tanh output WITH an action range is not what the reference computes)
inline int tanh_range_refusal(const char* entry, const mpg_cfg_t* cfg) {
    MPG_REQUIRE(!(cfg->policy_out_act == MPG_ACT_TANH && cfg->action_range > 0.f), "%s: tanh policy with an action range", entry);
    return MPG_OK;
}

// what the entry points of the MODEL-BACKED env (model_rollout.hip: mpg_model_env_*, mpg_worker_rollout_model) ask of a cfg: the double
// pendulum, the one kind without a real env - the two kinds that have one are sent to their entry points -, its widths, and no tanh
// output under an action range
inline int model_env_cfg_refusal(const char* entry, const mpg_cfg_t* cfg) {
    MPG_REQUIRE(cfg, "%s: null configuration", entry);
    MPG_REQUIRE(cfg->env_kind != MPG_ENV_PATH_TRACKING && cfg->env_kind != MPG_ENV_INVERTED_PENDULUM,
                "%s: env kind %d has a real env (mpg_env_* and the worker entry points on it); the model-backed env is the double pendulum's",
                entry, cfg->env_kind);
    MPG_REQUIRE(cfg->env_kind == MPG_ENV_INVERTED_DOUBLE_PENDULUM, "%s: unknown env kind %d (the model-backed env: 2 double pendulum)", entry,
                cfg->env_kind);
    MPG_REQUIRE(cfg->obs_dim == 11, "%s: the double-pendulum model env has obs_dim 11 (got %d)", entry, cfg->obs_dim);
    MPG_REQUIRE(cfg->act_dim == 1, "%s: the double-pendulum model env has act_dim 1 (got %d)", entry, cfg->act_dim);
    MPG_REQUIRE(!(cfg->policy_out_act == MPG_ACT_TANH && cfg->action_range > 0.f), "%s: tanh policy with an action range", entry);
    return MPG_OK;
}

// ... and of the agent count, the episode limit and - `ring` not null - the ring position (pointers are judged before this)
inline int model_env_size_refusal(const char* entry, int n, int max_steps, const RingPtrs* ring, int capacity, int next_idx) {
    MPG_REQUIRE(n > 0, "%s: no agents (n %d)", entry, n);
    MPG_REQUIRE(max_steps >= 0, "%s: max_steps >= 0, 0 for no episode limit (got %d)", entry, max_steps);
    if (!ring) return MPG_OK;
    MPG_REQUIRE(capacity >= n, "%s: the ring's capacity %d is below n %d", entry, capacity, n);
    MPG_REQUIRE(next_idx >= 0 && next_idx < capacity, "%s: next_idx %d outside [0, capacity %d)", entry, next_idx, capacity);
    return MPG_OK;
}

// what the step -> ring entry points ask of the agent count and the ring
inline bool ring_ok(int n, int capacity, int next_idx, const RingPtrs& ring) {
    return n > 0 && capacity >= n && next_idx >= 0 && next_idx < capacity && ring.obs && ring.act && ring.rew && ring.obs2 && ring.done;
}

// the four worker rollouts: `pointers` - the entry point's own non-null ones -, the ring, and `iters` iterations of n transitions in it
inline int ring_rollout_refusal(const char* entry, bool pointers, int n, int iters, int capacity, int next_idx, const RingPtrs& ring) {
    MPG_REQUIRE(pointers && ring.obs && ring.act && ring.rew && ring.obs2 && ring.done, "%s: null pointer", entry);
    MPG_REQUIRE(ring_ok(n, capacity, next_idx, ring), "%s: bad ring (n %d, capacity %d < n, or next_idx %d outside it)", entry, n, capacity,
                next_idx);
    MPG_REQUIRE(iters >= 1, "%s: iters >= 1 (got %d)", entry, iters);
    // (what bounds one launch's run time; the reference's worker runs 64, its pendulum worker 512)
    MPG_REQUIRE(iters <= 1024, "%s: iters <= 1024 (got %d)", entry, iters);
    // two iterations would write one slot from different workgroups with no order between them
    MPG_REQUIRE((long)iters * n <= capacity, "%s: iters * n = %ld transitions do not fit the ring's capacity %d", entry, (long)iters * n,
                capacity);
    return MPG_OK;
}

// the two evaluation rollouts: n agents, `steps` steps, `pointers` - all of them but the nullable done flags
inline int eval_rollout_refusal(const char* entry, int n, int steps, bool pointers) {
    MPG_REQUIRE(n > 0, "%s: no agents (n %d)", entry, n);
    MPG_REQUIRE(steps >= 1, "%s: steps >= 1 (got %d)", entry, steps);
    // (what bounds one launch's run time; the parsers' largest fixed_steps is 500)
    MPG_REQUIRE(steps <= 1024, "%s: steps <= 1024 (got %d)", entry, steps);
    MPG_REQUIRE(pointers, "%s: null pointer", entry);
    return MPG_OK;
}

namespace cart_pole {   // env_cart_pole.hip: analytic RK4 statement of inverted_pendulum_conti.xml
int reset_from_obs(int n, int obs_dim, float* state, const float* init_obs, hipStream_t s);
int reset(int n, int obs_dim, float* state, const uint8_t* done_mask, uint64_t seed, uint64_t ctr, float* obs, hipStream_t s);
int step(int n, int obs_dim, float* state, const float* action, float* obs, float* reward, uint8_t* done, uint8_t* done_intended,
         hipStream_t s);
int step_store_reset(int n, int obs_dim, float* state, const float* action, int capacity, int next_idx, const RingPtrs& ring,
                     uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out, hipStream_t s);
}  // namespace cart_pole
