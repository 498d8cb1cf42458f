/* Host loops of tools/bench_ndpg.py: the two samplers enqueued natively, `reps` times back to back, so that neither is charged an
 * interpreter or a foreign-function call per launch.  The entry points come in as pointers (the tool resolves them in the engine's
 * library), so this file links against nothing.
 *
 *   cc -O2 -shared -fPIC -Iinclude tools/bench_ndpg_chain.c -o tools/bench_ndpg_chain.so      (bench_ndpg.py does this itself) */
#include "mpg_hip.h"

typedef int (*reset_fn)(int, int, int, float*, const float*, mpg_stream_t);
typedef int (*policy_fn)(const mpg_cfg_t*, const float*, int, const float*, float, uint64_t, uint64_t, float*, mpg_stream_t);
typedef int (*step_fn)(int, int, int, float*, const float*, float*, float*, uint8_t*, uint8_t*, mpg_stream_t);
typedef int (*rollout_fn)(const mpg_cfg_t*, const float*, int, int, const float*, const float*, float*, float*, mpg_stream_t);

/* the sequence of mpg_step_begin for MPG-v1 (train_step.cpp, "MPGLearner.sample"): 1 + 2 n - 1 launches */
int bench_chain(reset_fn reset, policy_fn policy_action, step_fn env_step, const mpg_cfg_t* cfg, const float* policy, int rows, int n,
                const float* obs0, const float* act0, float* state, float* obs, float* act, float* rewards, uint8_t* done,
                uint8_t* done_intended, mpg_stream_t s, int reps) {
    const int kind = cfg->env_kind, od = cfg->obs_dim;
    for (int r = 0; r < reps; ++r) {
        int rc = reset(kind, rows, od, state, obs0, s);
        if (rc) return rc;
        for (int t = 0; t < n; ++t) {
            const float* a = act0;
            if (t > 0) {
                rc = policy_action(cfg, policy, rows, obs, 0.f, 0, 0, act, s);
                if (rc) return rc;
                a = act;
            }
            rc = env_step(kind, rows, od, state, a, obs, rewards + (size_t)t * rows, done, done_intended, s);
            if (rc) return rc;
        }
    }
    return 0;
}

int bench_launch(rollout_fn rollout, const mpg_cfg_t* cfg, const float* policy, int rows, int n, const float* obs0, const float* act0,
                 float* rewards, float* last_obs, mpg_stream_t s, int reps) {
    for (int r = 0; r < reps; ++r) {
        int rc = rollout(cfg, policy, rows, n, obs0, act0, rewards, last_obs, s);
        if (rc) return rc;
    }
    return 0;
}
