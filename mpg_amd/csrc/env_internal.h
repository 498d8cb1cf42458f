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

namespace cart_pole {   // env_cart_pole.hip: analytic RK4 statement of inverted_pendulum_conti.xml
int reset_from_obs(int n, int obs_dim, float* state, const float* init_obs, hipStream_t s);
int reset(int n, int obs_dim, float* state, const uint8_t* done_mask, uint64_t seed, uint64_t ctr, float* obs, hipStream_t s);
int step(int n, int obs_dim, float* state, const float* action, float* obs, float* reward, uint8_t* done, uint8_t* done_intended,
         hipStream_t s);
int step_store_reset(int n, int obs_dim, float* state, const float* action, int capacity, int next_idx, const RingPtrs& ring,
                     uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out, hipStream_t s);
}  // namespace cart_pole
