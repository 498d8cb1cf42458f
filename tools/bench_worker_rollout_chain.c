/* Host loops of tools/bench_worker_rollout.py: one worker sample as `iters` mpg_worker_step launches (what sample of
 * train_step.cpp enqueues without the one-launch form) and as one mpg_worker_rollout launch, `reps` samples back to back, so that
 * neither is charged an interpreter or a foreign-function call per launch (and the pendulum's forms of both, further down).  The entry points come in as pointers (the tool resolves
 * them in the engine's library), so this file links against nothing.
 *
 *   cc -O2 -shared -fPIC -Iinclude tools/bench_worker_rollout_chain.c -o tools/bench_worker_rollout_chain.so
 *   (bench_worker_rollout.py does this itself) */
#include "mpg_hip.h"

typedef int (*step_fn)(const mpg_cfg_t*, const float*, int, float*, float*, float, uint64_t, uint64_t, float*, int, int, float*, float*,
                       float*, float*, uint8_t*, uint64_t, uint64_t, uint8_t*, const mpg_replay_draw_t*, int, float*, float*, float*, float*,
                       mpg_stream_t);
typedef int (*rollout_fn)(const mpg_cfg_t*, const float*, int, int, float*, float*, float, uint64_t, uint64_t, float*, int, int, float*,
                          float*, float*, float*, uint8_t*, uint64_t, uint64_t, uint8_t*, mpg_stream_t);

/* one side's buffers and counters; both forms advance them alike */
typedef struct {
    float *state, *obs, *act;
    float *ring_obs, *ring_act, *ring_rew, *ring_obs2;
    uint8_t *ring_done, *done;
    int capacity, next_idx;
    uint64_t ctr;
} worker_side_t;

int bench_chain(step_fn worker_step, const mpg_cfg_t* cfg, const float* policy, int n, int iters, float sigma, worker_side_t* w,
                mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r)
        for (int it = 0; it < iters; ++it) {
            int rc = worker_step(cfg, policy, n, w->state, w->obs, sigma, 11, w->ctr, w->act, w->capacity, w->next_idx, w->ring_obs,
                                 w->ring_act, w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->done, 0, 0, 0, 0, 0, 0, s);
            if (rc) return rc;
            w->ctr++;
            w->next_idx = (w->next_idx + n) % w->capacity;
        }
    return 0;
}

/* the pendulum's chain (bench_worker_rollout.py --env pendulum): two launches per iteration, mpg_policy_action + mpg_env_step_store_reset,
 * as sample's loop enqueues them; its one-launch form, mpg_worker_rollout_pendulum, has mpg_worker_rollout's signature and goes
 * through bench_launch */
typedef int (*action_fn)(const mpg_cfg_t*, const float*, int, const float*, float, uint64_t, uint64_t, float*, mpg_stream_t);
typedef int (*step_store_fn)(int, int, int, float*, const float*, int, int, float*, float*, float*, float*, uint8_t*, uint64_t, uint64_t,
                             float*, uint8_t*, mpg_stream_t);

int bench_chain_pendulum(action_fn policy_action, step_store_fn step_store_reset, const mpg_cfg_t* cfg, const float* policy, int n, int iters,
                         float sigma, worker_side_t* w, mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r)
        for (int it = 0; it < iters; ++it) {
            int rc = policy_action(cfg, policy, n, w->obs, sigma, 11, w->ctr, w->act, s);
            if (rc) return rc;
            rc = step_store_reset(MPG_ENV_INVERTED_PENDULUM, n, 4, w->state, w->act, w->capacity, w->next_idx, w->ring_obs, w->ring_act,
                                  w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->obs, w->done, s);
            if (rc) return rc;
            w->ctr++;
            w->next_idx = (w->next_idx + n) % w->capacity;
        }
    return 0;
}

int bench_launch(rollout_fn worker_rollout, const mpg_cfg_t* cfg, const float* policy, int n, int iters, float sigma, worker_side_t* w,
                 mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r) {
        int rc = worker_rollout(cfg, policy, n, iters, w->state, w->obs, sigma, 11, w->ctr, w->act, w->capacity, w->next_idx, w->ring_obs,
                                w->ring_act, w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->done, s);
        if (rc) return rc;
        w->ctr += (uint64_t)iters;
        w->next_idx = (int)(((long)w->next_idx + (long)iters * n) % w->capacity);
    }
    return 0;
}

/* the pendulum's chain under the tanh-squashed Gaussian policy (bench_worker_rollout.py --env pendulum --stochastic): three calls per
 * iteration, mpg_normal_fill + mpg_policy_sample_squashed (two launches) + mpg_env_step_store_reset, against its one-launch form,
 * mpg_worker_sample_rollout_pendulum; eps / logp [n] and the workspace are the caller's */
typedef int (*normal_fill_fn)(int, uint64_t, uint64_t, float*, mpg_stream_t);
typedef int (*sample_squashed_fn)(const mpg_cfg_t*, const float*, int, const float*, const float*, float*, float*, float*, void*, size_t,
                                  mpg_stream_t);
typedef int (*sample_rollout_fn)(const mpg_cfg_t*, const float*, int, int, float*, float*, uint64_t, uint64_t, float*, int, int, float*,
                                 float*, float*, float*, uint8_t*, uint64_t, uint64_t, uint8_t*, mpg_stream_t);

int bench_chain_sample_pendulum(normal_fill_fn normal_fill, sample_squashed_fn policy_sample, step_store_fn step_store_reset,
                                const mpg_cfg_t* cfg, const float* policy, int n, int iters, float* eps, float* logp, void* ws,
                                size_t ws_bytes, worker_side_t* w, mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r)
        for (int it = 0; it < iters; ++it) {
            int rc = normal_fill(n, 11, w->ctr, eps, s);
            if (rc) return rc;
            rc = policy_sample(cfg, policy, n, w->obs, eps, w->act, logp, 0, ws, ws_bytes, s);
            if (rc) return rc;
            rc = step_store_reset(MPG_ENV_INVERTED_PENDULUM, n, 4, w->state, w->act, w->capacity, w->next_idx, w->ring_obs, w->ring_act,
                                  w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->obs, w->done, s);
            if (rc) return rc;
            w->ctr++;
            w->next_idx = (w->next_idx + n) % w->capacity;
        }
    return 0;
}

int bench_launch_sample(sample_rollout_fn sample_rollout, const mpg_cfg_t* cfg, const float* policy, int n, int iters, worker_side_t* w,
                        mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r) {
        int rc = sample_rollout(cfg, policy, n, iters, w->state, w->obs, 11, w->ctr, w->act, w->capacity, w->next_idx, w->ring_obs,
                                w->ring_act, w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->done, s);
        if (rc) return rc;
        w->ctr += (uint64_t)iters;
        w->next_idx = (int)(((long)w->next_idx + (long)iters * n) % w->capacity);
    }
    return 0;
}

/* PathTracking under a stochastic policy (bench_worker_rollout.py --stochastic): the plain Gaussian head's chain is what
 * sample's loop enqueues, one mpg_worker_sample_step per iteration; the squashed head has no one-launch step, its chain is
 * the three calls per iteration (mpg_normal_fill over 2 n elements + mpg_policy_sample_squashed + mpg_env_step_store_reset: four
 * launches).  Both against mpg_worker_sample_rollout through bench_launch_sample. */
typedef int (*sample_step_fn)(const mpg_cfg_t*, const float*, int, float*, float*, uint64_t, uint64_t, float*, float*, int, int, float*, float*,
                              float*, float*, uint8_t*, uint64_t, uint64_t, uint8_t*, mpg_stream_t);

int bench_chain_sample_step(sample_step_fn sample_step, const mpg_cfg_t* cfg, const float* policy, int n, int iters, worker_side_t* w,
                            mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r)
        for (int it = 0; it < iters; ++it) {
            int rc = sample_step(cfg, policy, n, w->state, w->obs, 11, w->ctr, w->act, 0, w->capacity, w->next_idx, w->ring_obs, w->ring_act,
                                 w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->done, s);
            if (rc) return rc;
            w->ctr++;
            w->next_idx = (w->next_idx + n) % w->capacity;
        }
    return 0;
}

int bench_chain_sample(normal_fill_fn normal_fill, sample_squashed_fn policy_sample, step_store_fn step_store_reset, const mpg_cfg_t* cfg,
                       const float* policy, int n, int iters, float* eps, float* logp, void* ws, size_t ws_bytes, worker_side_t* w,
                       mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r)
        for (int it = 0; it < iters; ++it) {
            int rc = normal_fill(n * cfg->act_dim, 11, w->ctr, eps, s);
            if (rc) return rc;
            rc = policy_sample(cfg, policy, n, w->obs, eps, w->act, logp, 0, ws, ws_bytes, s);
            if (rc) return rc;
            rc = step_store_reset(cfg->env_kind, n, cfg->obs_dim, w->state, w->act, w->capacity, w->next_idx, w->ring_obs, w->ring_act,
                                  w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->obs, w->done, s);
            if (rc) return rc;
            w->ctr++;
            w->next_idx = (w->next_idx + n) % w->capacity;
        }
    return 0;
}

/* the model-backed double pendulum env (bench_worker_rollout.py --env model): two launches per iteration, mpg_policy_action +
 * mpg_model_env_step_store_reset, as sample's loop enqueues them, against mpg_worker_rollout_model.  The side's `state` is the agents'
 * step counts (int32 [n]); max_steps is the episode limit */
typedef int (*model_step_store_fn)(const mpg_cfg_t*, int, float*, const float*, int, int*, int, int, float*, float*, float*, float*, uint8_t*,
                                   uint64_t, uint64_t, uint8_t*, mpg_stream_t);
typedef int (*model_rollout_fn)(const mpg_cfg_t*, const float*, int, int, float*, int*, int, float, uint64_t, uint64_t, float*, int, int, float*,
                                float*, float*, float*, uint8_t*, uint64_t, uint64_t, uint8_t*, mpg_stream_t);

int bench_chain_model(action_fn policy_action, model_step_store_fn step_store_reset, const mpg_cfg_t* cfg, const float* policy, int n, int iters,
                      int max_steps, float sigma, worker_side_t* w, mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r)
        for (int it = 0; it < iters; ++it) {
            int rc = policy_action(cfg, policy, n, w->obs, sigma, 11, w->ctr, w->act, s);
            if (rc) return rc;
            rc = step_store_reset(cfg, n, w->obs, w->act, max_steps, (int*)w->state, w->capacity, w->next_idx, w->ring_obs, w->ring_act,
                                  w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->done, s);
            if (rc) return rc;
            w->ctr++;
            w->next_idx = (w->next_idx + n) % w->capacity;
        }
    return 0;
}

int bench_launch_model(model_rollout_fn worker_rollout, const mpg_cfg_t* cfg, const float* policy, int n, int iters, int max_steps, float sigma,
                       worker_side_t* w, mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r) {
        int rc = worker_rollout(cfg, policy, n, iters, w->obs, (int*)w->state, max_steps, sigma, 11, w->ctr, w->act, w->capacity, w->next_idx,
                                w->ring_obs, w->ring_act, w->ring_rew, w->ring_obs2, w->ring_done, 4, w->ctr, w->done, s);
        if (rc) return rc;
        w->ctr += (uint64_t)iters;
        w->next_idx = (int)(((long)w->next_idx + (long)iters * n) % w->capacity);
    }
    return 0;
}
