/* Host loops of tools/bench_sac_native.py: the stochastic worker step as the three stand-alone calls and as the one launch, enqueued
 * natively `reps` times back to back over a ring that advances, so that neither is charged an interpreter or a foreign-function call
 * per launch.  The entry points come in as pointers (the tool resolves them in the engine's library), so this file links against
 * nothing.
 *
 *   cc -O2 -shared -fPIC -Iinclude tools/bench_sac_native_chain.c -o tools/bench_sac_native_chain.so   (bench_sac_native.py does this) */
#include "mpg_hip.h"

typedef int (*fill_fn)(int, uint64_t, uint64_t, float*, mpg_stream_t);
typedef int (*sample_fn)(const mpg_cfg_t*, const float*, int, const float*, const float*, float*, float*, float*, void*, size_t, mpg_stream_t);
typedef int (*store_fn)(int, int, int, float*, const float*, int, int, float*, float*, float*, float*, uint8_t*, uint64_t, uint64_t, float*,
                        uint8_t*, mpg_stream_t);
typedef int (*one_fn)(const mpg_cfg_t*, const float*, int, float*, float*, uint64_t, uint64_t, float*, float*, int, int, float*, float*,
                      float*, float*, uint8_t*, uint64_t, uint64_t, uint8_t*, mpg_stream_t);

typedef struct {
    float *state, *obs, *eps, *act, *logp;
    float *ring_obs, *ring_act, *ring_rew, *ring_obs2;
    uint8_t *ring_done, *done;
    void* ws;
    size_t ws_bytes;
    int capacity;
} bench_bufs_t;

/* what sample (train_step.cpp) enqueues where it takes the chain: 4 launches per step */
int bench_chain(fill_fn fill, sample_fn sample, store_fn store, const mpg_cfg_t* cfg, const float* policy, int n, const bench_bufs_t* b,
                uint64_t ctr0, mpg_stream_t s, int reps) {
    int next = 0;
    for (int r = 0; r < reps; ++r) {
        int rc = fill(2 * n, 11, ctr0 + r, b->eps, s);
        if (rc) return rc;
        rc = sample(cfg, policy, n, b->obs, b->eps, b->act, b->logp, 0, b->ws, b->ws_bytes, s);
        if (rc) return rc;
        rc = store(cfg->env_kind, n, cfg->obs_dim, b->state, b->act, b->capacity, next, b->ring_obs, b->ring_act, b->ring_rew, b->ring_obs2,
                   b->ring_done, 13, ctr0 + r, b->obs, b->done, s);
        if (rc) return rc;
        next = (next + n) % b->capacity;
    }
    return 0;
}

int bench_launch(one_fn one, const mpg_cfg_t* cfg, const float* policy, int n, const bench_bufs_t* b, uint64_t ctr0, mpg_stream_t s, int reps) {
    int next = 0;
    for (int r = 0; r < reps; ++r) {
        int rc = one(cfg, policy, n, b->state, b->obs, 11, ctr0 + r, b->act, 0, b->capacity, next, b->ring_obs, b->ring_act, b->ring_rew,
                     b->ring_obs2, b->ring_done, 13, ctr0 + r, b->done, s);
        if (rc) return rc;
        next = (next + n) % b->capacity;
    }
    return 0;
}
