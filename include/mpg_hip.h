/*
 * mpg_hip.h - C ABI of libmpg_hip.so, the MI355X (gfx950) drop-in for the data-parallel hot path of
 * idthanm/mpg (Mixed Policy Gradient).
 *
 * The reference has no FFI: its "plugin API" is a set of duck-typed Python classes picked through
 * registries (train_scripts/train_script.py:39-51, envs_and_models/__init__.py:13-15).  Each entry point
 * below replaces the arithmetic of one group of those methods; the file:line it replaces is cited on
 * every declaration (paths relative to the reference root).  The python package mpg_amd keeps the reference's class and
 * method names on top of this ABI; INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor), contiguous float32
 *     unless stated; nothing is allocated, freed or copied to the host behind the caller's back;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued on it and
 *     the call returns immediately (no host synchronisation);
 *   - return value: 0 on success, a negative MPG_E* code or -(hipError_t) otherwise; no exceptions cross
 *     the boundary;
 *   - re-entrant per (device, stream): no global mutable state (caches and timers are caller-owned handles, see
 *     mpg_wcache_t / mpg_prof_t; hyper-parameters arrive in mpg_cfg_t, never through the environment);
 *   - networks are 2-hidden-layer ELU MLPs with 256 hidden units (model.py:20-43), parameters stored as
 *     ONE flat float32 vector in Keras order  W1[in][256] b1[256] W2[256][256] b2[256] W3[256][out] b3[out]
 *     (kernels row-major (in,out), exactly `Model.get_weights()` flattened);
 *   - row batches (obs, act, ...) are row-major [rows][dim] like the reference's numpy arrays.
 */
#ifndef MPG_HIP_H
#define MPG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mpg_stream_t; /* hipStream_t */

enum {
    MPG_OK = 0,
    MPG_EINVAL = -1000,   /* bad argument (null pointer, unsupported dimension, ...) */
    MPG_EWORKSPACE = -1001 /* workspace too small: call the *_workspace_bytes query */
};

enum { MPG_ENV_PATH_TRACKING = 0, MPG_ENV_INVERTED_PENDULUM = 1, MPG_ENV_INVERTED_DOUBLE_PENDULUM = 2 };
enum { MPG_ACT_LINEAR = 0, MPG_ACT_TANH = 1 };
enum { MPG_HIDDEN = 256 };
/* floats per agent of the opaque env state block, stored SoA [MPG_ENV_STATE_DIM][n]:
 * v_x, v_y, r, y, phi, x (veh_full_state) + delta_y, delta_phi (the two derived entries of veh_state). */
enum { MPG_ENV_STATE_DIM = 8 };

/* ABI version of this header; bumped on any signature change. */
int mpg_abi_version(void);
/* Human-readable description of the last error on this thread ("" if none). */
const char* mpg_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Caller-owned handles (no reference counterpart).  The library keeps NO process-wide mutable state: the packed
 * weight images and the optional kernel timer below are objects the caller creates, owns and passes in (through
 * mpg_cfg_t or an explicit argument).  The one thing kept on the library side is the thread-local text behind
 * mpg_last_error().
 * ---------------------------------------------------------------------------------------------- */

/* Packed register images of the 256x256 hidden kernels ("weight cache", acceleration only).  Describes ONE flat
 * parameter vector `params` = [net0 | net1 | ...] (Keras order each) and a caller-owned device array `packed` of
 * mpg_weight_cache_floats(n_nets) floats holding, per network, the forward and the transposed image of W2 in the
 * order the lanes of the MLP engine consume them (1 KiB coalesced loads instead of strided ones).  Entry points that
 * are told about a descriptor (mpg_cfg_t.wcache, or their explicit `wcache` argument) and receive a pointer into
 * `params` use the images; results are bit-identical with and without them.  The descriptor itself is HOST memory,
 * read at call time.  Whoever writes `params` keeps `packed` current: mpg_adam_polyak / mpg_clip_adam_polyak do so
 * themselves for the descriptors they are given, anything else calls mpg_weight_cache_pack afterwards. */
typedef struct {
    const float* params;  /* device: base of the flat vector the images mirror */
    float* packed;        /* device: mpg_weight_cache_floats(n_nets) floats */
    int n_nets;           /* <= 8 */
    int in_dim[8], out_dim[8];
    int* status;          /* device, nullable: MPG_STATUS_* bits are OR-ed into it (see "Numerical envelope" below) */
} mpg_wcache_t;
size_t mpg_weight_cache_floats(int n_nets);
/* (re)builds both images of every network of `wc` from wc->params: one launch on `stream`. */
int mpg_weight_cache_pack(const mpg_wcache_t* wc, mpg_stream_t stream);

/* Numerical envelope of the hidden-layer engine and how leaving it is reported.  The 256 x 256 hidden-layer products run
 * on the f16 matrix pipe with every float32 operand split into two fp16 halves (hi + lo: 22-23 significant bits, exact
 * products, float32 accumulation; csrc/mlp_core.h).  Operands are pre-scaled by powers of two; what that leaves as the
 * supported range is
 *     |first hidden activation| < 4094           (enters the image as x * 16; fp16 ends at 65504)
 *     |any network parameter|   < 1023.5         (hidden kernels enter as W * 64; the bound also keeps the reverse layer's
 *                                                 row-scaled operands, <= 16 * out * |W3|, in range)
 * Gradients entering the reverse layer and the weight-gradient product are scaled by data-dependent powers of two (per row
 * / per chunk of rows) and have no envelope of their own.  Outside the range a result would silently be wrong (an fp16
 * infinity turns a whole row into NaN, which the ELU's median instruction then drops), so the library reports it: every
 * forward pass tracks the largest first-layer pre-activation it saw, every (re)pack of an image checks the parameters, and a
 * violation sets a bit in the caller's device-side status word (mpg_cfg_t.status / mpg_wcache_t.status; nullable = not
 * reported).  A parameter beyond the bound enters the image clamped to +-65504 / 64.  The word is sticky: the caller reads
 * and clears it (mpg_amd.PolicyWithQs.check_status raises on it); `-DMPG_F32_MFMA` builds the exact-fp32 engine, which has
 * no envelope.  Reference counterpart: none (TensorFlow computes in float32 throughout). */
enum {
    MPG_STATUS_ACTIVATION_RANGE = 1, /* a first-hidden-layer activation reached 4094: that row's outputs are invalid */
    MPG_STATUS_PARAMETER_RANGE = 2,  /* a parameter reached 1023.5: clamped in the packed image */
    MPG_STATUS_NAN = 4               /* a NaN went into or came out of a network forward pass (mpg_policy_action and the other
                                        cfg-carrying forward entry points) - worker.py:95-107 `judge_is_nan` on the processed
                                        observations and on the actions, evaluated on the device */
};

/* Optional per-kernel timing with HIP events recorded on the launch stream.  mpg_prof_create allocates every event
 * up front (2 * MPG_PROF_SLOTS * max_samples of them), so that nothing is created inside a timed region;
 * mpg_prof_start(p, every) clears the samples and records around every `every`-th launch of each slot from then on
 * (0: stop; an event record is a stream packet of its own and costs ~4-5 us between two otherwise back-to-back
 * kernels, so timing EVERY launch slows a 0.5 ms step by 6 %); mpg_prof_read waits for the recorded events of a slot
 * and returns their summed duration and count.  A timer takes effect on the calls made with a mpg_cfg_t whose `prof`
 * field points to it (and on the native step driver's env launch).  Slots: 0 k_rollout_fwd, 1 k_rollout_bwd,
 * 2 env step, 3 k_forward, 4 k_backward, 5 k_wgrad, 6 k_target_fused, 7 k_critic_fused, 8 the caller's gradient exchange
 * (mpg_prof_region_begin / _end around whatever the caller enqueues between mpg_step_begin and mpg_step_end: RCCL all-reduce or
 * the one-shot exchange; the reference's hand-over is optimizer.py:60-94), 9 k_clip_adam_polyak.  No reference counterpart
 * (the reference times with utils/misc.py:39-90 TimerStat on the host).  Not thread-safe: one timer per launching
 * thread. */
enum { MPG_PROF_SLOTS = 10 };
typedef struct mpg_prof mpg_prof_t;
int mpg_prof_create(int max_samples, mpg_prof_t** out);
int mpg_prof_destroy(mpg_prof_t* p);
int mpg_prof_start(mpg_prof_t* p, int every);
int mpg_prof_read(mpg_prof_t* p, int slot, double* total_ms, int* count);
const char* mpg_prof_slot_name(int slot);
/* time a caller-side region on `stream` under `slot` with the same every-n-th sampling (no-ops for a null or stopped timer) */
int mpg_prof_region_begin(mpg_prof_t* p, int slot, mpg_stream_t stream);
int mpg_prof_region_end(mpg_prof_t* p, int slot, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Vectorised real environment (K1)
 * ---------------------------------------------------------------------------------------------- */

/* Two real environments sit behind these entry points, selected by env_kind:
 *   MPG_ENV_PATH_TRACKING      PathTrackingEnv (path_tracking_env.py:356-487), act_dim 2, obs_dim = 6 + num_future_data
 *                              (0 <= num_future_data <= MPG_ENV_MAX_FUTURE): [v_x-20, v_y, r, dy, dphi, x | look-ahead
 *                              delta-y terms at x + k * 0.2 v_x, :385-402];
 *   MPG_ENV_INVERTED_PENDULUM  InvertedPendulumContiEnv (inverted_pendulum_conti.py:5-30 + inverted_pendulum_conti.xml) as
 *                              an analytic RK4 cart-pole (the reference steps it with MuJoCo, which cannot be pinned
 *                              here: csrc/env_cart_pole.hip), act_dim 1, obs_dim 4: [p, theta, pdot, thetadot].
 * state: the opaque block [MPG_ENV_STATE_DIM][n].
 *
 * MPG_ENV_INVERTED_DOUBLE_PENDULUM (2) names a differentiable MODEL only - InvertedDoublePendulumModel
 * (envs_and_models/inverted_double_pendulum_model.py:103-144), the third model the reference registers
 * (envs_and_models/__init__.py:12-15) - as mpg_cfg_t.env_kind of the rollout entry points (mpg_rollout_pg, mpg_rollout_q_target,
 * mpg_rollout_q_estimation and their workspace queries):
 *   observation  obs_dim 11: [p, sin t1, sin t2, cos t1, cos t2, pdot, t1dot, t2dot, frc1, frc2, frc3] (:105).  A START observation
 *                (the caller's batch) carries whatever the env put into the three constraint-force entries, and all 11 entries reach
 *                the first policy / critic evaluation; its state is [p, atan2(sin t1, cos t1), atan2(sin t2, cos t2), pdot, t1dot,
 *                t2dot] (:126-132).  Every MODEL observation is that function of the model state with zeros in entries 8..10.
 *   action       act_dim 1, force u = 500 a (:143-144); one step = five explicit-Euler sub-steps of 0.01 s of f_xu_old (:26-53), the
 *                reward (:89-100) on the state behind them.  The angles are not wrapped.
 *   noise        none: `eps`, noise_seed and noise_ctr are accepted and unused for this model.
 *   limits       exactly (obs_dim 11, act_dim 1, env_kind 2): every other triple with one of these values is MPG_EINVAL (workspace
 *                queries: 0).  The 3 x 3 mass-matrix system is solved in closed form where the reference calls tf.linalg.inv.
 * The REAL env is gym's MuJoCo InvertedDoublePendulum-v2 and is not provided: mpg_env_reset_from_obs, mpg_env_reset, mpg_env_step,
 * mpg_env_step_store_reset(_draw) and mpg_worker_step return MPG_EINVAL for env_kind 2 with a message that says so, and the native
 * step driver, whose first act is to sample the real env, REFUSES a context with this env_kind in mpg_step_begin before anything
 * is enqueued (NADP on this model runs through the rollout entry points on caller-supplied batches). */
enum { MPG_ENV_MAX_FUTURE = 10 };

/* env.reset(init_obs=...)  - path_tracking_env.py:410-421 / DummyVecEnv.reset(init_obs=) for the pendulum.
 * Rebuilds the full state of all n agents from init_obs [n][obs_dim] (PathTracking reads its six base entries). */
int mpg_env_reset_from_obs(int env_kind, int n, int obs_dim, float* state, const float* init_obs, mpg_stream_t stream);

/* env.reset()  - path_tracking_env.py:423-454.  Re-draws every agent whose done_mask byte is
 * non-zero (done_mask == NULL: all agents) from the reset law x~U(0,600), dy~N(0,1), dphi~N(0,pi/9),
 * v_x~U(15,25), beta~N(0,.15), v_y=v_x tan(beta), r~N(0,.3) (pendulum: U(-0.01, 0.01) on all four,
 * inverted_pendulum_conti.py:21-25) with a counter-based Philox4x32-10 stream
 * keyed by (seed, call counter ctr, agent index); writes obs [n][obs_dim] for ALL agents. */
int mpg_env_reset(int env_kind, int n, int obs_dim, float* state, const uint8_t* done_mask, uint64_t seed, uint64_t ctr,
                  float* obs, mpg_stream_t stream);

/* PathTrackingEnv.step  - path_tracking_env.py:456-487 with VehicleDynamics.simulation :144-179 (20
 * sub-steps at 200 Hz), compute_rewards :181-199 (on the pre-step state), judge_done :474-487.
 * action [n][2] in [-1,1] (scaled by [1.2pi/9, 3] and clipped inside, :457-459); outputs obs [n][obs_dim],
 * reward [n], done [n] bytes.  done follows the reference literally and is therefore always 1
 * (SURVEY.md B-0); done_intended (nullable) receives the evidently intended |alpha| > |bound| test.
 * Pendulum: inverted_pendulum_conti.py:9-19, action [n][1] clipped to +-3, 2 RK4 steps of 0.02 s, real done flag.
 * A NaN action is handed on (NaN state, observation and reward, done 1), infinite ones are +-3. */
int mpg_env_step(int env_kind, int n, int obs_dim, float* state, const float* action, float* obs, float* reward,
                 uint8_t* done, uint8_t* done_intended, mpg_stream_t stream);

/* The inner body of OffPolicyWorker.sample after the policy (worker.py:108-112) in one launch: env.step, the
 * transition (obs, action, RAW reward, obs', done) written straight into the replay ring at (next_idx + i) % capacity
 * (ReplayBuffer.add, buffer.py:46-55), then env.reset() of the agents whose done flag is set
 * (path_tracking_env.py:445) with the Philox stream (seed, ctr).  Same results as mpg_env_step + mpg_replay_add +
 * mpg_env_reset.  obs_out [n][obs_dim]: the observations after the reset; done_out (nullable) [n]. */
int mpg_env_step_store_reset(int env_kind, int n, int obs_dim, float* state, const float* action, int capacity, int next_idx,
                             float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                             uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out, mpg_stream_t stream);

/* out[i] = ((slots[0][i] + slots[1][i]) + slots[2][i]) + ...  - the local sum of the one-shot all-reduce (SURVEY.md 8 f4;
 * mpg_amd/dist.py OneShotAllReduce): every rank of a node holds the ranks' gradient buffers in `n_slots` staging slots of
 * `n` floats and adds them in rank order, so that all replicas compute the same association.  Replaces the arithmetic of
 * the gradient exchange, optimizer.py:60-94 (there: one learner's gradients applied at a time). */
int mpg_sum_slots(const float* slots, int n_slots, int n, float* out, mpg_stream_t stream);
/* The same sum over a SLICE of the slots: slot r starts at slots + r * slot_stride (floats), n <= slot_stride entries are summed.
 * The reduce half of the two-shot (reduce-scatter + all-gather) form of the exchange: rank r sums only its 1/world slice, in the
 * same rank order, and distributes the result (mpg_amd/dist.py OneShotAllReduce, mode 'twoshot'; optimizer.py:60-94). */
int mpg_sum_slots_strided(const float* slots, int n_slots, size_t slot_stride, int n, float* out, mpg_stream_t stream);
/* The same sum with the clip's partial sums of squares of the RESULT as a by-product (round 6, ABI 10): sq_part[k*MPG_CLIP_PARTS + b]
 * exactly as mpg_sq_partials(out, seg_sizes, n_seg, ...) would compute them - the same bits - so that an exchanged gradient
 * (optimizer.py:60-94) reaches mpg_clip_adam_polyak / mpg_step_end (mpg_train_ctx_t.clip_partials_ready) without another pass over it.
 * seg_sizes[0..n_seg) (host): the networks at the head of the buffer; the n - sum(seg_sizes) floats behind them (statistics) are
 * summed too.  n_slots = 1: a copy with the partials (the gather array of the two-shot form). */
int mpg_sum_slots_sq(const float* slots, int n_slots, size_t slot_stride, int n, float* out, const int* seg_sizes, int n_seg,
                     float* sq_part /* n_seg * MPG_CLIP_PARTS floats */, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Networks (K3), critic targets, losses and gradients (K5, K6)
 * ---------------------------------------------------------------------------------------------- */

/* Per-call options of the gradient entry points, reached through mpg_cfg_t.grad_opts (NULL: none).  HOST memory, read at
 * call time.  No reference counterpart: it only changes HOW the same numbers are scheduled. */
typedef struct {
    void* critics_ready_event;           /* hipEvent_t, nullable.  mpg_mpg_gradients then finishes the critics' gradient (chunk
                                            products + slab sums + loss sums) BEFORE the reverse sweep and records this event behind
                                            it on the launch stream: a caller that exchanges gradients between GPUs can start the
                                            critics' part of the exchange on a second stream under the reverse sweep
                                            (optimizer.py:60-94, payload mpg_learner.py:448-455).  Costs one launch more. */
} mpg_grad_opts_t;

/* Hyper-parameters of one config (host memory, read at call time). */
typedef struct {
    int obs_dim, act_dim;       /* path tracking: 6 + num_future_data (0 <= num_future_data <= MPG_ENV_MAX_FUTURE = 10), 2;
                                   pendulum: 4, 1; double pendulum (model only): 11, 1.  LIMIT: the reference accepts any num_future_data
                                   (path_tracking_env.py:385-402); every entry point returns MPG_EINVAL for obs_dim > 16 (first
                                   layers: policy up to 16 wide, critics up to 24; obs_scale[16]) */
    int policy_out_act;         /* MPG_ACT_TANH (train_script.py:267) or MPG_ACT_LINEAR (train_script4mujoco.py:371) */
    float action_range;         /* <= 0: none; pendulum 3.0 -> a = range*tanh(mean) (policy.py:197-199) */
    float obs_scale[16];        /* 'scale' preprocessor, preprocessor.py:142-143 (train_script.py: [1,1,2,1,2.4,1/1200] + [1]*num_future_data) */
    float rew_scale, rew_shift; /* preprocessor.py:155-157 */
    float gamma;                /* 0.98 */
    int env_kind;               /* differentiable model used by the rollout: MPG_ENV_* */
    /* optional caller-owned handles (NULL: none) */
    const mpg_wcache_t* wcache[2]; /* packed images of up to two parameter vectors (e.g. networks, targets) that calls
                                      made with this cfg may receive pointers into */
    mpg_prof_t* prof;           /* kernel timer that the calls made with this cfg report to */
    int* status;                /* device, nullable: MPG_STATUS_* bits are OR-ed into it by the forward passes made with this cfg */
    const mpg_grad_opts_t* grad_opts; /* nullable: scheduling options of mpg_mpg_gradients (above) */
} mpg_cfg_t;

/* MLPNet.call  - model.py:39-43:  y[rows][out_used] = act(ELU(ELU(x W1 + b1) W2 + b2) W3 + b3)[:, :out_used].
 * x [rows][in_dim] (supported (in_dim, out_used): (6,2) (8,1) (4,1) (5,1) (6,1), the look-ahead widths, and (6..16, 4):
 * all four logits of the PathTracking policy head); the first n_scaled input
 * columns are multiplied by in_scale[] (host array, may be NULL). */
int mpg_mlp_forward(const float* params, int in_dim, int out_dim, int out_used, int out_act, int rows,
                    const float* x, const float* in_scale, int n_scaled, float* y,
                    const mpg_wcache_t* wcache /* nullable */, mpg_stream_t stream);

/* PolicyWithQs.compute_action / compute_target_action, deterministic branch  - policy.py:193-217:
 * act[rows][act_dim] = mean half of the policy output on obs*obs_scale (x action_range*tanh if set).
 * explore_sigma > 0 adds N(0, sigma) per element from Philox(seed, ctr) - OffPolicyWorker.sample,
 * worker.py:96-98. */
int mpg_policy_action(const mpg_cfg_t* cfg, const float* policy_params, int rows, const float* obs,
                      float explore_sigma, uint64_t seed, uint64_t ctr, float* act, mpg_stream_t stream);

/* MPGLearner.compute_clipped_double_q_target  - learners/mpg_learner.py:126-134 (q2t != NULL), the 1-step
 * target of :148-152 (q2t == NULL), and TD3Learner.compute_clipped_double_q_target learners/td3.py:69-81 when
 * smooth_eps [rows][act_dim] (standard normal) is given: a' += clip(sigma*eps, -c, c) (no re-clipping).
 *   y = (rew+shift)*scale + gamma * min_i Qt_i(s~', a'),  a' = pi_t(s~').  No done mask. */
size_t mpg_q_targets_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_q_targets(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, const float* q2t, int rows,
                  const float* rew, const float* obs_tp1, const float* smooth_eps, float smooth_sigma,
                  float smooth_clip, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* TD3Learner.get_batch_data with a prioritized buffer (learners/td3.py:94-101): the clipped double-Q target y (td3.py:69-81,
 * as mpg_q_targets with smooth_eps) AND the plain Q1 target y1 of the priorities' td error (td3.py:83-92: y1 = r~ + gamma
 * Q1t(s~', pi_t(s~'))) from ONE evaluation of the target policy.  Same values as the two mpg_q_targets calls.  Workspace:
 * mpg_q_targets_workspace_bytes. */
int mpg_td3_targets(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, const float* q2t, int rows,
                    const float* rew, const float* obs_tp1, const float* smooth_eps, float smooth_sigma,
                    float smooth_clip, float* y, float* y1, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* out[0 .. n) ~ N(0, 1) from Philox4x32-10(seed, ctr) + Box-Muller: the target-policy smoothing noise of TD3 (td3.py:74,
 * tf.random.normal in the reference) without a framework kernel; the same (seed, ctr) gives the same numbers in the native step
 * driver and in the method-by-method path. */
int mpg_normal_fill(int n, uint64_t seed, uint64_t ctr, float* out, mpg_stream_t stream);

/* TD3Learner.compute_td_error (td3.py:83-92) finished from what the step already has: out = (y1 - y) - td with td = Q1(s~, a) - y
 * from mpg_q_loss_grad and (y, y1) from mpg_td3_targets; signed (mpg_per_update takes |.| + eps). */
int mpg_td3_priority_errors(int rows, const float* y1, const float* y, const float* td, float* out, mpg_stream_t stream);

/* n-step return of MPG-v1 (mpg_learner.py:155-169) once the real-env rollout exists (mpg_env_step x n):
 *   y = sum_t gamma^t r~_t + gamma^n Q1t(s~_n, pi_t(s~_n)).  rewards [n][rows] RAW, last_obs [rows][obs_dim].
 * Workspace: mpg_q_targets_workspace_bytes. */
int mpg_nstep_targets(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, int rows, int n,
                      const float* rewards, const float* last_obs, float* y, void* ws, size_t ws_bytes,
                      mpg_stream_t stream);

/* The same for InvertedPendulumConti-v0, whose bootstrap value the reference clips (mpg_learner.py:163-164:
 * all_values_tp1 = clip_by_value(all_values_tp1, -0.5, 0.)):
 *   y = sum_t gamma^t r~_t + gamma^n min(max(Q1t(s~_n, pi_t(s~_n)), q_lo), q_hi).
 * mpg_nstep_targets' launches with the clip in the last one, its workspace (mpg_q_targets_workspace_bytes) and its refusals under this
 * entry point's name; refused too, with a text of its own each: a bound that is not finite, q_lo > q_hi.  A NaN value stays NaN, as
 * TF's minimum / maximum hand it on.  mpg_nstep_targets itself keeps its kernel and its bits.
 * (added without a signature change elsewhere: the ABI version stays 10) */
#define MPG_PENDULUM_NSTEP_Q_LO (-0.5f) /* mpg_learner.py:163-164 */
#define MPG_PENDULUM_NSTEP_Q_HI (0.f)
int mpg_nstep_targets_clipped(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, int rows, int n,
                              const float* rewards, const float* last_obs, float q_lo, float q_hi,
                              float* y, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* MPGLearner.q_forward_and_backward  - mpg_learner.py:326-354 (also td3.py:103-118, nadp.py:173-184), ONE critic:
 *   L = 0.5 * mean_B (Q(s~,a) - y)^2 and dL/dtheta_Q.
 * inv_b_global = 1/B_global (the mean's divisor; 1/rows on one GPU).  Outputs: loss_sum[0] = this GPU's share
 * of L, grad = flat gradient (68353 floats path tracking) reduced over this GPU's rows and NOT clipped,
 * td (nullable) [rows] = Q(s~,a) - y. */
size_t mpg_q_loss_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_q_loss_grad(const mpg_cfg_t* cfg, const float* q_params, int rows, const float* obs, const float* act,
                    const float* y, float inv_b_global, float* loss_sum, float* grad, float* td, void* ws,
                    size_t ws_bytes, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * n-step model rollout + mixed policy gradient (K2+K3+K4)
 * ---------------------------------------------------------------------------------------------- */

/* MPGLearner.model_rollout_for_policy_update + policy_forward_and_backward  - learners/mpg_learner.py:226-286,
 * :356-365 (default flags: deriv_interval_policy=False - parameter gradients flow only through the step-0
 * action) and, with all_steps_param_grad != 0, the NADP variant learners/nadp.py:128-171,
 * :186-194 where every step goes through pi_theta (needs rows*M % 16 == 0).
 *
 *   rows   B_local start states obs0 [rows][obs_dim]  (the M copies are tiled inside: trajectory = m*rows + b)
 *          PathTracking start states are taken as they are, like the reference takes them: any v_x (the clamp to [1, 35],
 *          path_tracking_env.py:289, applies to every state the MODEL produces, and the adjoint of v_x is zero across a clamped
 *          step) and any heading error the float32 sine accepts - a start observation is NOT wrapped into (-pi, pi], every model
 *          state is (:290-291).  Tested with v_x at both ends of the clamp and |heading error| up to 3.5
 *          (tests/test_model_edges_gpu.py); the pendulum's angle is not range-limited.
 *   eps    [n][M*rows] standard-normal draws for the model's injected noise
 *          (path_tracking_env.py:119: dy += 0.5 + 0.01 eps; inverted_pendulum_model.py:61: p += 0.1 + 0.5 eps);
 *          NULL: drawn inside the kernel from Philox4x32-10 keyed by (noise_seed, noise_ctr, step, trajectory)
 *   select/n_select/w (HOST arrays, n_select <= 4)   slices k whose mean returns R_k = mean(G_k + gamma^k Q1)
 *          enter the loss  sum_k w_k * (-R_k)   (w = rule_based_weights, mpg_learner.py:384-399, computed by the host)
 *   inv_b_global   1/B_global: divisor of the batch mean (the M-mean is applied inside); n < 32
 * Outputs
 *   ret_sum [n_select], ret_sqsum [n_select]: sum over this GPU's rows of the M-mean return and of its square
 *   grad    flat policy gradient (68612 floats path tracking) of the loss, reduced over this GPU's rows, NOT clipped.
 * Look-ahead observations (cfg->obs_dim > 6, num_future_data of path_tracking_env.py:246-270): the start observation's
 * look-ahead entries are inputs, every model observation's are copies of delta_y (:262-268) and their adjoint folds into
 * delta_y's; any M and either parameter-gradient mode (round 4). */
size_t mpg_rollout_pg_workspace_bytes(const mpg_cfg_t* cfg, int rows, int M, int n, int n_select,
                                      int all_steps_param_grad);
int mpg_rollout_pg(const mpg_cfg_t* cfg, const float* policy_params, const float* q1_params, int rows, int M,
                   int n, const int* select, int n_select, const float* w, const float* obs0, const float* eps,
                   uint64_t noise_seed, uint64_t noise_ctr, float inv_b_global, int all_steps_param_grad, float* ret_sum, float* ret_sqsum, float* grad,
                   void* ws, size_t ws_bytes, mpg_stream_t stream);

/* AMPCLearner.model_rollout_for_policy_update + policy_forward_and_backward  - learners/ampc.py:73-96: the policy-only learner.
 * n policy evaluations and model steps from obs0 (M copies tiled inside, like mpg_rollout_pg), NO critic and no policy
 * evaluation at the last observation; every step goes through pi_theta.  The rewards are summed WITHOUT a discount whatever
 * cfg->gamma holds (ampc.py:83; the parser's gamma = 1 only reaches the Preprocessor).
 *   eps    [n][M*rows] standard-normal model noise, or NULL: Philox4x32-10 keyed by (noise_seed, noise_ctr, step, trajectory)
 * Outputs
 *   ret_sum [1], ret_sqsum [1]: sum over this GPU's rows of the M-mean reward sum and of its square
 *   grad    flat policy gradient of  -inv_b_global / M * sum(rewards_sum), reduced over this GPU's rows, NOT clipped.
 * Needs rows*M % 16 == 0 and 0 < n < 32; all three models of mpg_rollout_pg.  Composed from that entry point's launches: the
 * forward sweep with the single slice n, k_ampc_returns (the sums, and zeros where the reverse sweep reads the critic's input
 * gradient), the reverse sweep, the weight-gradient launch over n + 1 steps (the last one contributes exact zeros).
 * (added without a signature change elsewhere: the ABI version stays 10) */
size_t mpg_ampc_pg_workspace_bytes(const mpg_cfg_t* cfg, int rows, int M, int n);
int mpg_ampc_pg(const mpg_cfg_t* cfg, const float* policy_params, int rows, int M, int n, const float* obs0, const float* eps,
                uint64_t noise_seed, uint64_t noise_ctr, float inv_b_global, float* ret_sum, float* ret_sqsum, float* grad,
                void* ws, size_t ws_bytes, mpg_stream_t stream);

/* MPGLearner.compute_gradient without the clip, as one entry point  - learners/mpg_learner.py:401-431:
 * target (when y_in == NULL: clipped double-Q target from target_params, :126-134), critic losses and gradients of
 * the n_q (1: MPG-v1, 2: MPG-v2) critics (:326-354), n-step model rollout + mixed policy gradient (:226-286,356-365).
 * params / target_params / grad: flat [Q1 | (Q2) | policy] like PolicyWithQs.models (policy.py:72-86); y_in: optional
 * precomputed targets [rows] (MPG-v1's real-env n-step return); y_out [rows] receives the targets used.
 * stats (16 floats): [0..n_q) critic losses, [2..2+n_select) return sums, [2+n_select..2+2 n_select) sums of squares.
 * Everything is this GPU's UN-clipped partial, scaled by inv_b_global = 1/B_global: all-reduce, then
 * mpg_clip_by_global_norm.  Same results as mpg_q_targets + mpg_q_loss_grad + mpg_rollout_pg (up to the association
 * of the slab sums) in 6 launches instead of 22 when rows % 16 == 0 and M == 1; otherwise it calls those.
 * sq_part (nullable, (n_q+1)*MPG_CLIP_PARTS floats): on a single GPU the last launch also leaves the clip's partial sums
 * of squares of `grad` there (what mpg_sq_partials would compute), ready for mpg_clip_adam_polyak. */
/* Optional fused minibatch draw: ReplayBuffer.sample (buffer.py:70-78) from the device ring, the same draw as
 * mpg_replay_sample_uniform(n_storage, rows, seed, ctr, ...).  With `draw` != NULL the obs / act / rew / obs_tp1
 * arguments of mpg_mpg_gradients are OUTPUTS: the minibatch is gathered inside the first launch (one launch less per
 * iteration) and left there, the indices in idx_out and the dones (as float) in done_out (both nullable). */
typedef struct {
    int n_storage;                    /* transitions currently stored */
    uint64_t seed, ctr;               /* Philox key / counter of this draw (ctr = ReplayBuffer.replay_times) */
    const float *ring_obs, *ring_act, *ring_rew, *ring_obs2;
    const uint8_t* ring_done;
    int* idx_out;
    float* done_out;
    /* pre_gathered != 0: mpg_env_step_store_reset_draw already gathered every drawn row whose ring slot lies OUTSIDE the
     * window [fresh_start, fresh_start + fresh_count) mod capacity (the slots that launch was writing) into the output
     * arrays; only rows drawn from the window are gathered now.  Same minibatch either way. */
    int pre_gathered, capacity, fresh_start, fresh_count;
} mpg_replay_draw_t;

/* mpg_env_step_store_reset plus, in spare workgroups of the same launch, the gather of the NEXT minibatch draw
 * (draw->n_storage = the ring size after this add, draw->seed / ctr = that draw's Philox key and counter): the random
 * ring reads (one DRAM line and one page-table walk per array and row) then overlap the 20 sub-steps of the env instead
 * of sitting at the head of mpg_mpg_gradients' first launch.  Rows drawn from the slots this launch writes are skipped;
 * pass the same draw with pre_gathered = 1, fresh_start = next_idx, fresh_count = n to mpg_mpg_gradients.
 * Path-tracking env with obs_dim 6 only (MPG_EINVAL otherwise). */
int mpg_env_step_store_reset_draw(int env_kind, int n, int obs_dim, float* state, const float* action, int capacity, int next_idx,
                                  float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                                  uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out /* nullable */,
                                  const mpg_replay_draw_t* draw, int rows, float* b_obs, float* b_act, float* b_rew,
                                  float* b_obs2, mpg_stream_t stream);

/* OffPolicyWorker.sample's inner body (worker.py:95-112) as ONE launch for the path-tracking env, cfg->obs_dim = 6 + num_future_data
 * in 6 .. 16 (obs_dim 7 .. 16: the policy's 16-wide first layer), act_dim 2:
 * mpg_policy_action (deterministic action + N(0, explore_sigma) noise keyed by noise_seed / noise_ctr, written to act_out [n][2])
 * followed by mpg_env_step_store_reset (draw == NULL) or mpg_env_step_store_reset_draw - the policy pass of a 16-agent group by one
 * workgroup, whose first wave then steps those agents.  obs_io [n][obs_dim]: the current observations in, the next ones out; the
 * ring's observation arrays have rows of obs_dim entries.  Actions, ring rows, env state and observations are bit-identical to the
 * two stand-alone calls'.  draw != NULL serves obs_dim 6 only, like mpg_env_step_store_reset_draw (the pre-gathered rows feed the
 * fused gradient launch, which exists for six-entry observations only): MPG_EINVAL with obs_dim > 6, and for any other env / width. */
int mpg_worker_step(const mpg_cfg_t* cfg, const float* policy_params, int n, float* state, float* obs_io, float explore_sigma,
                    uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity, int next_idx, float* ring_obs,
                    float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done, uint64_t env_seed, uint64_t env_ctr,
                    uint8_t* done_out /* nullable */, const mpg_replay_draw_t* draw /* nullable */, int rows, float* b_obs,
                    float* b_act, float* b_rew, float* b_obs2, mpg_stream_t stream);

/* OffPolicyWorker.sample's loop (worker.py:91-119: `iters` = batch_size / num_agent iterations of policy -> + N(0, explore_sigma) ->
 * env.step -> ring -> env.reset) as ONE launch for the path-tracking env, obs_dim 6 .. 16, act_dim 2: one workgroup keeps a 16-agent
 * group's policy weights and agents in registers for all iterations; global memory is read at the start only (weights, state, obs_io)
 * and written, never read back.  Everything these `iters` consecutive calls leave behind, it = 0 .. iters - 1,
 *   mpg_worker_step(cfg, policy_params, n, state, obs_io, explore_sigma, noise_seed, noise_ctr + it, act_out, capacity,
 *                   (next_idx + it * n) % capacity, ring..., env_seed, env_ctr + it, done_out, draw = NULL, ...);
 * is bit-identical: state, obs_io [n][obs_dim] (the current observations in, those after the last iteration out), act_out [n][2] and
 * done_out [n] (nullable) of the LAST iteration, every ring array - iteration `it` writes the slots (next_idx + it * n + i) % capacity -
 * and the sticky status word.  The counters are 64-bit sums (the carry into the high word included).  There is no pre-gathered draw.
 * Refused before any launch with MPG_EINVAL, "mpg_worker_rollout" and a text of its own each, the outputs untouched: what
 * mpg_worker_step refuses (a null configuration, another env - env_kind 2 with the text of the other real-env entry points -, obs_dim
 * outside 6 .. 16, act_dim != 2, a tanh policy with an action range, a null pointer other than done_out, n <= 0, capacity < n,
 * next_idx outside [0, capacity)), iters < 1, iters > 1024 (what bounds one launch's run time; the reference's worker runs 64) and
 * iters * n > capacity (two iterations would write one slot from different workgroups with no order between them).
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_worker_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                       float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity, int next_idx,
                       float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done, uint64_t env_seed,
                       uint64_t env_ctr, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* The same for the pendulum's real env (MPG_ENV_INVERTED_PENDULUM, obs_dim 4, act_dim 1; the reference's pendulum worker runs ONE agent
 * for 512 iterations per sample): one workgroup keeps a 16-agent group's policy weights in registers and one agent per lane for all
 * iterations.  This env's done flag is real: an agent is carried across iterations until it falls and is re-drawn.  Everything these
 * `iters` consecutive pairs leave behind, it = 0 .. iters - 1,
 *   mpg_policy_action(cfg, policy_params, n, obs_io, explore_sigma, noise_seed, noise_ctr + it, act_out, stream);
 *   mpg_env_step_store_reset(MPG_ENV_INVERTED_PENDULUM, n, 4, state, act_out, capacity, (next_idx + it * n) % capacity, ring...,
 *                            env_seed, env_ctr + it, obs_io, done_out, stream);
 * is bit-identical: state, obs_io [n][4] (the current observations in, those after the last iteration out), act_out [n][1] and
 * done_out [n] (nullable) of the LAST iteration, every ring array - iteration `it` writes the slots (next_idx + it * n + i) % capacity -
 * and the sticky status word.  The counters are 64-bit sums (the carry into the high word included).  Deterministic policy only
 * (action_range * tanh(mean) where the cfg has an action range).
 * Refused before any launch with MPG_EINVAL, "mpg_worker_rollout_pendulum" and a text of its own each, the outputs untouched: a null
 * configuration, env_kind 2 (the text of the other real-env entry points), any other env that is not the pendulum, obs_dim != 4,
 * act_dim != 1, a tanh policy with an action range, a null pointer other than done_out, n <= 0, capacity < n, next_idx outside
 * [0, capacity), iters < 1, iters > 1024 and iters * n > capacity.
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_worker_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                                float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity, int next_idx,
                                float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done, uint64_t env_seed,
                                uint64_t env_ctr, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* The pendulum's worker sample for the TANH-SQUASHED Gaussian policy (SAC with an action range; worker.py:96: the action is the
 * sample, a = action_range * tanh(mean + sigma * eps)) as ONE launch, with mpg_worker_rollout_pendulum's residency: one workgroup per
 * 16-agent group, the policy's weights in registers, one agent per lane for all iterations.  Everything these `iters` consecutive
 * triples leave behind, it = 0 .. iters - 1,
 *   mpg_normal_fill(n, sample_seed, sample_ctr + it, eps, stream);
 *   mpg_policy_sample_squashed(cfg, policy_params, n, obs_io, eps, act_out, logp, NULL, ws, ws_bytes, stream);
 *   mpg_env_step_store_reset(MPG_ENV_INVERTED_PENDULUM, n, 4, state, act_out, capacity, (next_idx + it * n) % capacity, ring...,
 *                            env_seed, env_ctr + it, obs_io, done_out, stream);
 * is bit-identical: state, obs_io [n][4], act_out [n][1] and done_out [n] (nullable) of the LAST iteration, every ring array and the
 * sticky status word (the activation-range and NaN reports of the policy pass).  Agent i draws element i of iteration it's stream
 * inside the launch (no eps array exists); both counters are 64-bit sums.  There is no explore_sigma, as for mpg_worker_sample_step,
 * and no log-density output: the worker discards it and the ring has no column for it.
 * Refused before any launch with MPG_EINVAL, "mpg_worker_sample_rollout_pendulum" and a text of its own each, the outputs untouched:
 * a null configuration, env_kind 2 (the text of the other real-env entry points), any other env that is not the pendulum (PathTracking
 * with an action range included), what the squashed entry points refuse of a cfg (act_dim != 1, no positive finite action range, a
 * tanh output activation, obs_dim != 4), a null pointer other than done_out, n <= 0, capacity < n, next_idx outside [0, capacity),
 * iters < 1, iters > 1024 and iters * n > capacity.
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_worker_sample_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                                       uint64_t sample_seed, uint64_t sample_ctr, float* act_out, int capacity, int next_idx,
                                       float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                                       uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* OffPolicyWorker.sample's inner body for a STOCHASTIC policy (worker.py:95-112 with the action sampled from the Gaussian head below,
 * no explore_sigma) as ONE launch for the path-tracking env, obs_dim 6 .. 16, act_dim 2.  Bit-identical - actions, log-densities,
 * every ring row, env state, next observations, done flags and the sticky status word - to
 *   mpg_normal_fill(2 n, sample_seed, sample_ctr, eps);
 *   mpg_policy_sample(cfg, policy_params, n, obs_io, eps, act_out, logp_out, NULL, ...);
 *   mpg_env_step_store_reset(MPG_ENV_PATH_TRACKING, n, obs_dim, state, act_out, capacity, next_idx, ring..., env_seed, env_ctr,
 *                            obs_io, done_out);
 * row r draws elements 2 r and 2 r + 1 of that stream inside the launch (no eps array exists).  There is no pre-gathered minibatch
 * draw and no explore_sigma.  Refused before any launch with MPG_EINVAL and "mpg_worker_sample_step" in the message: everything
 * mpg_policy_sample refuses (null pointers - logp_out alone may be null -, n <= 0, act_dim != 2, another env, action_range > 0, an
 * unsupported width), a ring that mpg_worker_step refuses (capacity < n, next_idx outside [0, capacity)), and env_kind 2 with the
 * text of the other real-env entry points. */
int mpg_worker_sample_step(const mpg_cfg_t* cfg, const float* policy_params, int n, float* state, float* obs_io,
                           uint64_t sample_seed, uint64_t sample_ctr, float* act_out, float* logp_out /* nullable */,
                           int capacity, int next_idx, float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2,
                           uint8_t* ring_done, uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out /* nullable */,
                           mpg_stream_t stream);

/* OffPolicyWorker.sample's loop for a STOCHASTIC policy on the path-tracking env (obs_dim 6 .. 16, act_dim 2) as ONE launch, with
 * mpg_worker_rollout's residency: one workgroup keeps a 16-agent group's policy weights (all four output columns) and agents in
 * registers for all iterations; global memory is read at the start only and written, never read back.  Both heads: the plain Gaussian
 * one (no action range) and the tanh-squashed one (cfg->action_range > 0 over a linear output: a = action_range * tanh(mean + sigma *
 * eps)).  Everything these `iters` consecutive triples leave behind, it = 0 .. iters - 1,
 *   mpg_normal_fill(2 n, sample_seed, sample_ctr + it, eps, stream);
 *   mpg_policy_sample(cfg, policy_params, n, obs_io, eps, act_out, logp, NULL, ws, ws_bytes, stream);      (no action range)
 *   mpg_policy_sample_squashed(... the same arguments ...);                                                (with one)
 *   mpg_env_step_store_reset(MPG_ENV_PATH_TRACKING, n, obs_dim, state, act_out, capacity, (next_idx + it * n) % capacity, ring...,
 *                            env_seed, env_ctr + it, obs_io, done_out, stream);
 * is bit-identical: state, obs_io [n][obs_dim], act_out [n][2] and done_out [n] (nullable) of the LAST iteration, every ring array -
 * iteration `it` writes the slots (next_idx + it * n + i) % capacity, no other slot is touched - and the sticky status word (the
 * activation-range and NaN reports of the policy pass).  Without an action range that is also `iters` calls of mpg_worker_sample_step.
 * Row r draws elements 2 r and 2 r + 1 of iteration it's stream inside the launch (no eps array exists); both counters are 64-bit
 * sums.  There is no explore_sigma and no log-density output: the worker discards it and the ring has no column for it.
 * Refused before any launch with MPG_EINVAL, "mpg_worker_sample_rollout" and a text of its own each, the outputs untouched: a null
 * configuration, env_kind 2 (the text of the other real-env entry points), any other env that is not PathTracking, obs_dim outside
 * 6 .. 16, act_dim != 2 (in the order of the other seven one-launch rollouts), with an action range what the squashed entry points refuse of it (a tanh output activation, a range that
 * is not finite), a null pointer other than done_out, n <= 0, capacity < n, next_idx outside [0, capacity), iters < 1, iters > 1024
 * and iters * n > capacity.
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_worker_sample_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                              uint64_t sample_seed, uint64_t sample_ctr, float* act_out, int capacity, int next_idx,
                              float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                              uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* MPGLearner.sample / NDPGLearner.sample - learners/mpg_learner.py:109-124, learners/ndpg.py:99-114, PathTracking env, ONE launch:
 * from obs0 [rows][obs_dim] take n real-env steps, the first with the replay action act0 [rows][2], the later ones with the ONLINE
 * policy's deterministic action (no noise, no reset on done).  rewards [n][rows] RAW, last_obs [rows][obs_dim].  Bit-identical - the
 * sticky status word included - to mpg_env_reset_from_obs followed by, for t < n, mpg_policy_action(explore_sigma 0) when t > 0 and
 * mpg_env_step; no env state block, action or done array is needed.  obs_dim 6 .. 16, act_dim 2, 1 <= n < 32: MPG_EINVAL otherwise,
 * for any other env and for a tanh policy with an action range. */
int mpg_env_rollout(const mpg_cfg_t* cfg, const float* policy_params, int rows, int n, const float* obs0, const float* act0,
                    float* rewards, float* last_obs, mpg_stream_t stream);

/* MPGLearner.sample - learners/mpg_learner.py:85-105 - for InvertedPendulumConti-v0, ONE launch: from obs0 [rows][4] take n real-env
 * steps, the first with the replay action act0 [rows], the later ones with the ONLINE policy's deterministic action (no noise; `done`
 * is ignored and nothing is reset).  rewards [n][rows] RAW, last_obs [rows][4].  Bit-identical - the sticky status word included - to
 * mpg_env_reset_from_obs followed by, for t < n, mpg_policy_action(explore_sigma 0) when t > 0 and mpg_env_step, for both weight
 * forms (packed image and strided); no env state block, action or done array is needed.
 * Refused before any launch with MPG_EINVAL, "mpg_env_rollout_pendulum" and a text of its own each: a null configuration, env_kind 2
 * (the text of the other real-env entry points), any other env that is not the pendulum, obs_dim != 4, act_dim != 1, n < 1, n > 1024,
 * rows <= 0, a null pointer, a tanh output activation with an action range.
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_env_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int rows, int n, const float* obs0, const float* act0,
                             float* rewards, float* last_obs, mpg_stream_t stream);

/* Evaluator.run_n_episodes_parallel's loop - evaluator.py:132-139 - on the path-tracking env (obs_dim 6 .. 16, act_dim 2) as ONE launch:
 * from the env's own state [MPG_ENV_STATE_DIM][n] and its current observations obs_io [n][obs_dim] take `steps` steps with the policy's
 * deterministic action (compute_mode: explore_sigma 0; for a stochastic stack the mean columns under the cfg's output rule).  `done` is
 * not consulted, nothing is reset, and the action goes to the env unclipped and is recorded unclipped.  Everything these `steps`
 * consecutive pairs leave behind, t = 0 .. steps - 1,
 *   mpg_policy_action(cfg, policy_params, n, obs_io, 0, 0, 0, act_traj + t * n * 2, stream);         (obs_io recorded at obs_traj + t * n * obs_dim first)
 *   mpg_env_step(MPG_ENV_PATH_TRACKING, n, obs_dim, state, act_traj + t * n * 2, obs_io, rew_traj + t * n, done_out, done_intended_out, stream);
 * is bit-identical: obs_traj [steps][n][obs_dim] (the observations BEFORE each step), act_traj [steps][n][2], rew_traj [steps][n] RAW,
 * state, obs_io and the done flags of the LAST step (both nullable), and the sticky status word - for both weight forms (packed image and
 * strided).  One workgroup keeps a 16-agent group's policy weights and agents in registers for all steps; global memory is read at the
 * start only and written, never read back.
 * Refused before any launch with MPG_EINVAL, "mpg_eval_rollout" and a text of its own each, the outputs untouched: a null configuration,
 * env_kind 2 (the text of the other real-env entry points), any other env that is not PathTracking, obs_dim outside 6 .. 16, act_dim != 2,
 * n <= 0, steps < 1, steps > 1024 (what bounds one launch's run time; the parsers' largest fixed_steps is 500), a null pointer other than
 * the done flags, a tanh output activation with an action range.
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_eval_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int steps, float* state, float* obs_io,
                     float* obs_traj, float* act_traj, float* rew_traj, uint8_t* done_out /* nullable */,
                     uint8_t* done_intended_out /* nullable */, mpg_stream_t stream);

/* The same for the pendulum's real env (MPG_ENV_INVERTED_PENDULUM, obs_dim 4, act_dim 1): `steps` consecutive pairs of mpg_policy_action
 * (explore_sigma 0) and mpg_env_step as ONE launch, bit-identical in obs_traj [steps][n][4], act_traj [steps][n][1], rew_traj [steps][n],
 * state, obs_io, done_out (nullable; the last step's) and the status word.  An agent beyond the done bound keeps stepping, as in the chain.
 * obs_io and obs_traj are read and written four floats at a time: both must be 16-byte aligned (as mpg_env_step asks of its pendulum
 * observations; any device allocation is).
 * Refused before any launch with MPG_EINVAL, "mpg_eval_rollout_pendulum" and a text of its own each: a null configuration, env_kind 2,
 * any other env that is not the pendulum, obs_dim != 4, act_dim != 1, n <= 0, steps < 1, steps > 1024, a null pointer other than
 * done_out, a tanh output activation with an action range. */
int mpg_eval_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int n, int steps, float* state, float* obs_io,
                              float* obs_traj, float* act_traj, float* rew_traj, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* Evaluator.metrics_for_an_episode - evaluator.py:160-211 - for each of the n episodes of a recorded evaluation, and the mean of every
 * metric over the episodes (:153-156), as ONE launch.  Rows in the reference's key_list order:
 *   MPG_ENV_PATH_TRACKING (K = 8): episode_return, episode_len, delta_y_mse (obs column 3), delta_phi_mse (4), delta_v_mse (0),
 *     stationary_rew_mean (the rewards from step 20 on; NaN = 0 / 0 with steps <= 20), steer_mse (action 0 * 1.2 * pi / 9, operator by operator), acc_mse
 *     (action 1 * 3);
 *   MPG_ENV_INVERTED_PENDULUM (K = 18): episode_return, episode_len, x_mean, x_var, theta_mean, theta_var, xdot_mean, xdot_var,
 *     thetadot_mean, thetadot_var, x_mse, theta_mse, xdot_mse, thetadot_mse and the four _mse_25 over the first min(25, steps) steps.
 * The `_mse` are ROOT mean squares, as in the reference; variances are two-pass population variances.  Every float32 entry is widened
 * to double first and all arithmetic is double.  per_episode [K][n], mean [K] (device memory).  Sums run t ascending, then episode
 * ascending, without atomics: two launches give the same bits.
 * MPG_EINVAL for another env kind, n <= 0, steps < 1, an obs_dim that is not the kind's (6 .. 16; 4) and a null pointer.  The
 * pendulum's obs_traj is read four floats at a time and must be 16-byte aligned; per_episode and mean 8-byte, as doubles are. */
#define MPG_EVAL_METRICS_PATH_TRACKING 8
#define MPG_EVAL_METRICS_PENDULUM 18
int mpg_eval_metrics(int env_kind, int n, int steps, int obs_dim, const float* obs_traj, const float* act_traj, const float* rew_traj,
                     double* per_episode /* [K][n] */, double* mean /* [K] */, mpg_stream_t stream);

/* ---- The differentiable models on their own (the model side of what mpg_eval_rollout records on the env) ----
 * ONE rollout_out of the model cfg->env_kind names, for `rows` independent rows, as ONE elementwise launch (one lane per row): what the
 * forward sweep of the rollout entry points computes per step, with the same device functions.
 *   MPG_ENV_PATH_TRACKING (obs_dim 6 .. 16, act_dim 2): PathTrackingModel at 10 Hz.  The observation is taken as given - delta_phi is not
 *     wrapped on the way in, the look-ahead entries 6 .. of the input are not read - and every look-ahead entry of obs_next is a copy of
 *     its delta_y (entry 3), as in every MODEL observation.  Model noise: delta_y += 0.5 + 0.01 eps.
 *   MPG_ENV_INVERTED_PENDULUM (4, 1): InvertedPendulumModel; p += 0.1 + 0.5 eps.
 *   MPG_ENV_INVERTED_DOUBLE_PENDULUM (11, 1): InvertedDoublePendulumModel.  The state is atan2 of the observation's sines and cosines,
 *     as the sweeps take a start observation; obs_next holds the 11 features of the new state (entries 8 .. 10 zero).  No model noise:
 *     eps is not read.  This kind is SERVED here: the model is what exists of this env.
 * obs [rows][obs_dim], act [rows][act_dim] (taken as given, nothing is clipped beyond what the model clips), eps [rows] standard normal
 * or NULL = zeros (the noise terms at their means), obs_next [rows][obs_dim], rew [rows] RAW (before rew_shift / rew_scale).  The status
 * word of cfg is not touched.
 * Refused before any launch with MPG_EINVAL, "mpg_model_step" and a text of its own each, the outputs untouched: a null configuration,
 * an unknown env kind, an obs_dim / act_dim that is not the kind's, rows <= 0, a null pointer other than eps, a tanh output activation
 * with an action range (the cfg no entry point takes).
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_model_step(const mpg_cfg_t* cfg, int rows, const float* obs, const float* act, const float* eps /* nullable */, float* obs_next,
                   float* rew, mpg_stream_t stream);

/* A policy's closed loop on the model - inverted_double_pendulum_model.py:245-265: model.reset(obs), then compute_action -> rollout_out
 * `steps` times - as ONE launch, for n independent trajectories from obs0 [n][obs_dim].  Everything these `steps` consecutive pairs leave
 * behind, t = 0 .. steps - 1 with o_0 = obs0,
 *   mpg_policy_action(cfg, policy_params, n, o_t, 0, 0, 0, act_traj + t * n * act_dim, stream);
 *   mpg_model_step(cfg, n, o_t, act_traj + t * n * act_dim, eps ? eps + t * n : NULL, o_{t+1}, rew_traj + t * n, stream);
 * is bit-identical: obs_traj [steps][n][obs_dim] = o_t (the observations BEFORE each step), act_traj [steps][n][act_dim], rew_traj
 * [steps][n] RAW, last_obs [n][obs_dim] = o_steps, and the sticky status word - for both weight forms (packed image and strided).  The
 * record's layout is mpg_eval_rollout's, so mpg_eval_metrics reads it as it stands.  For a stochastic stack the action is the mean
 * columns under the cfg's output rule.  There is no done flag, and nothing is clipped beyond what the model clips.  eps [steps][n]
 * standard normal, or NULL = zeros.  One workgroup keeps a 16-trajectory group's policy weights and observation rows in registers for all
 * steps; nothing the launch wrote is read back.
 * Refused before any launch with MPG_EINVAL, "mpg_model_rollout" and a text of its own each, the outputs untouched: a null configuration,
 * an unknown env kind, an obs_dim / act_dim that is not the kind's (6 .. 16 / 2; 4 / 1; 11 / 1), n <= 0, steps < 1, steps > 1024 (what
 * bounds one launch's run time), a null pointer other than eps, a tanh output activation with an action range.
 * (added without a signature change elsewhere: the ABI version stays 10) */
int mpg_model_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int steps, const float* obs0, const float* eps /* nullable */,
                      float* obs_traj, float* act_traj, float* rew_traj, float* last_obs, mpg_stream_t stream);

/* ---- The double pendulum's model as an ENVIRONMENT (MPG_ENV_INVERTED_DOUBLE_PENDULUM only) ----
 * The real InvertedDoublePendulum-v2 is MuJoCo and is not provided; what a worker steps here is the reference authors' own model of it
 * (mpg_model_step), made an env by this project's choice of a done law, an episode limit and a reset law.  The env is stateless in the
 * observation: its state is the 11-entry observation row plus one int32 step count per agent (`age`).  mpg_env_*, mpg_eval_* and the
 * native step driver keep refusing env kind 2.
 *   Step: obs_next and the RAW rew are bit for bit mpg_model_step's for (obs, act) - atan2 of the row's sines and cosines, five Euler
 *     sub-steps of f_xu_old with u = 500 a, the model's reward; no alive bonus, no action clip, no noise; entries 8 .. 10 of the new row
 *     are zero.
 *   Done: fell = !(tip_y > 1.0f) with tip_y = 0.6f * obs_next[3] + 0.6f * obs_next[4], two rounded products and one rounded sum (gym's
 *     done = y <= 1 on the model's tip height; upright is 1.2); negated so that a NaN row is done and is re-drawn.  truncated =
 *     max_steps > 0 && age + 1 >= max_steps (gym registers 1000 for this id; 0: no limit).  done = fell | truncated, one byte 0 / 1.
 *     age becomes age + 1, or 0 after a reset.
 *   Reset (the shape of gym's reset_model): p, theta1, theta2 ~ U(-0.1, 0.1), pdot, theta1dot, theta2dot ~ 0.1 N(0, 1) from
 *     Philox4x32-10 keyed (seed, ctr, agent); the row is the 11 features of that state (entries 8 .. 10 zero), age 0.
 * Known differences from MuJoCo beside the dynamics: the model's theta2 is an ABSOLUTE angle, and nothing bounds the cart position.
 * Every entry point below refuses before any launch with MPG_EINVAL, its own name and a text of its own each, the outputs untouched: a
 * null configuration, env kind 0 or 1 (they have a real env: mpg_env_*), an unknown env kind, obs_dim != 11, act_dim != 1, a tanh output
 * activation with an action range, a null pointer other than the nullable ones, n <= 0, max_steps < 0, and where there is a ring
 * capacity < n and next_idx outside [0, capacity).
 * (added without a signature change elsewhere: the ABI version stays 10)
 *
 * Re-draws the agents whose done_mask byte is not 0 (NULL: all n) into obs_io [n][11] and sets their age_io [n] to 0; an agent whose
 * byte is 0 is left untouched, bit for bit. */
int mpg_model_env_reset(const mpg_cfg_t* cfg, int n, float* obs_io, int* age_io, const uint8_t* done_mask /* nullable */, uint64_t seed,
                        uint64_t ctr, mpg_stream_t stream);

/* One env step of n agents: obs [n][11], act [n][1] -> obs_next [n][11], rew [n] RAW, done [n]; age_io [n] is advanced by one (the
 * caller resets the done agents: mpg_model_env_reset with done as the mask).  The status word of cfg is not touched. */
int mpg_model_env_step(const mpg_cfg_t* cfg, int n, const float* obs, const float* act, int max_steps, int* age_io, float* obs_next,
                       float* rew, uint8_t* done, mpg_stream_t stream);

/* mpg_env_step_store_reset for this env, ONE launch: the transition (obs, act, raw rew, obs', done) of agent i goes to ring slot
 * (next_idx + i) % capacity, done agents are then re-drawn keyed (seed, ctr), and obs_io [n][11] holds the rows after the reset.  It
 * leaves behind exactly what mpg_model_env_step + mpg_replay_add + mpg_model_env_reset(done_mask = done) leave, bit for bit: obs_io,
 * age_io, the five ring arrays and done_out [n] (nullable). */
int mpg_model_env_step_store_reset(const mpg_cfg_t* cfg, int n, float* obs_io, const float* act, int max_steps, int* age_io, int capacity,
                                   int next_idx, float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                                   uint64_t seed, uint64_t ctr, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* A worker sample on the model env as ONE launch, with mpg_worker_rollout_pendulum's residency: one workgroup keeps a 16-agent group's
 * policy weights in registers and one agent's row and age per lane for all iterations.  Everything these `iters` consecutive pairs
 * leave behind, it = 0 .. iters - 1,
 *   mpg_policy_action(cfg, policy_params, n, obs_io, explore_sigma, noise_seed, noise_ctr + it, act_out, stream);
 *   mpg_model_env_step_store_reset(cfg, n, obs_io, act_out, max_steps, age_io, capacity, (next_idx + it * n) % capacity, ring...,
 *                                  env_seed, env_ctr + it, done_out, stream);
 * is bit-identical: obs_io [n][11], age_io [n], act_out [n][1] and done_out [n] (nullable) of the LAST iteration, every ring array -
 * iteration `it` writes the slots (next_idx + it * n + i) % capacity - and the sticky status word, for both weight forms (packed image
 * and strided).  The counters are 64-bit sums (the carry into the high word included).  Deterministic policy only.
 * Refused as above, and: iters < 1, iters > 1024 (what bounds one launch's run time), iters * n > capacity. */
int mpg_worker_rollout_model(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* obs_io, int* age_io, int max_steps,
                             float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity, int next_idx,
                             float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done, uint64_t env_seed,
                             uint64_t env_ctr, uint8_t* done_out /* nullable */, mpg_stream_t stream);

/* ---- The MPC baseline, SLSQP form (mpc/main.py:75-165) ----
 * ModelPredictiveControl.cost_function for `rows` independent problems.  x0 [rows][6] = [v_x, v_y, r, delta_y, delta_phi, x] with
 * entry 0 the SPEED in m/s as compute_rew reads it (:133; not the env's v_x - 20), u [rows][horizon][2] NORMALISED controls.
 *   for i < horizon:  u_i = u[i] * (MPG_MPC_STEER_SCALE, MPG_MPC_ACC_SCALE);  cost -= compute_rew(x, u_i);  x = compute_next_obses(x, u_i)
 * (:160-163; compute_next_obses: f_xu at tau = 0.1, then v_x clipped to [1, 35] and delta_phi wrapped once into (-pi, pi], :145-154).
 * No model noise, no 20 m/s shift: this is not the rollout sweeps' model step.
 * mpg_mpc_cost_grad, ONE launch: cost [rows]; grad (nullable) [rows][horizon][2] = d cost / d u with respect to the NORMALISED controls
 * (the two scales included), by the hand adjoint of the step; a step whose raw v_x leaves [1, 35] passes no adjoint through v_x (the
 * gate of the rollout sweeps' adjoint); traj (nullable) [rows][horizon + 1][6] the states x_0 .. x_horizon.  cost is the same bits
 * whether grad and traj are asked for or not.  float32, the hardware reciprocal / sine / cosine as in the rollout sweeps (delta_phi of
 * x0 is expected within a few pi).  Entry 5 of the state (x) never reaches the cost.
 *
 * mpg_mpc_solve, ONE launch: minimises the cost over the box [-1, 1]^(2 horizon) for every row by the spectral projected gradient method
 * (Birgin, Martinez, Raydan, SIAM J. Optim. 10, 2000) with its non-monotone line search, constants below.
 *   setup: u = clamp(u_io, -1, 1), f and g there.
 *   iteration k < iters:  d = clamp(u - alpha g, -1, 1) - u;  f_max = max of the last MPG_MPC_SPG_M accepted costs;
 *     lambda = 1, 1/2, ... (at most MPG_MPC_SPG_HALVINGS halvings): the first u + lambda d with cost <= f_max + MPG_MPC_SPG_GAMMA lambda <g, d>
 *     is accepted;  s = u_new - u, y = g_new - g, alpha = <s, s> / <s, y> if <s, y> > 0 else MPG_MPC_SPG_ALPHA_MAX_STEP, clamped to
 *     [MPG_MPC_SPG_ALPHA_LO, MPG_MPC_SPG_ALPHA_HI];  the first alpha is MPG_MPC_SPG_ALPHA0.
 *     (the trial point is clamped into the box once more: u + (c - u) can round one ulp past c)
 *   A row stops when max_i |clamp(u - g, -1, 1) - u|_i <= tol (checked after the setup and after every accepted step; tol 0: never) or
 *   when its line search accepts nothing (a NaN cost included: every comparison is false); it keeps its last accepted u.  NaN passes
 *   through the clamps, as through np.clip, so a NaN in x0 [0 .. 4] or in the start point fails the first search: info -1.
 * u_io [rows][horizon][2]: start point in, solution out;  cost_out [rows] the last accepted cost (bit for bit mpg_mpc_cost_grad's at the
 * returned u);  pgnorm_out [rows] the norm above at that point;  info [rows]: the number of accepted iterations k, or -(k + 1) for a row
 * whose search failed after k of them.  Every loop has a fixed bound (iters, the halvings, horizon).  One lane per row, its arrays in LDS
 * (11 * horizon * 256 bytes per 64 rows); a row's result does not depend on which other rows share the launch.
 *
 * Both refuse before any launch with MPG_EINVAL, their own name and a text of its own each, the outputs untouched: rows <= 0, horizon < 1,
 * horizon > MPG_MPC_MAX_HORIZON, (solve) iters < 0, iters > MPG_MPC_MAX_ITERS, a negative or NaN tol, a null pointer other than grad / traj.
 * (added without a signature change elsewhere: the ABI version stays 10) */
#define MPG_MPC_MAX_HORIZON 31         /* the rollout entry points' bound (n < 32) */
#define MPG_MPC_MAX_ITERS 1000
#define MPG_MPC_STEER_SCALE 0.4f       /* main.py:161 */
#define MPG_MPC_ACC_SCALE 3.0f
#define MPG_MPC_SPG_M 5                /* non-monotone memory */
#define MPG_MPC_SPG_HALVINGS 20
#define MPG_MPC_SPG_GAMMA 1e-4f        /* sufficient decrease */
#define MPG_MPC_SPG_ALPHA0 0.05f
#define MPG_MPC_SPG_ALPHA_MAX_STEP 10.0f /* the step taken when <s, y> <= 0 */
#define MPG_MPC_SPG_ALPHA_LO 1e-6f
#define MPG_MPC_SPG_ALPHA_HI 1e3f
int mpg_mpc_cost_grad(int rows, int horizon, const float* x0 /* [rows][6] */, const float* u /* [rows][horizon][2] */,
                      float* cost /* [rows] */, float* grad /* nullable, [rows][horizon][2] */,
                      float* traj /* nullable, [rows][horizon + 1][6] */, mpg_stream_t stream);
int mpg_mpc_solve(int rows, int horizon, int iters, float tol, const float* x0, float* u_io /* start point in, solution out */,
                  float* cost_out /* [rows] */, float* pgnorm_out /* [rows] */, int* info /* [rows] */, mpg_stream_t stream);

/* ---- MPC on the learners' OWN models ----
 * The undiscounted horizon cost of a control sequence on the model cfg->env_kind names - the three models of mpg_model_step, the ones
 * NADP, AMPC and MPG's policy half differentiate through; NOT mpg_mpc_*'s problem above - for `rows` independent start rows:
 *   s_0 = the model's reading of obs0's row, exactly as the sweeps and mpg_model_rollout take a START observation: PathTracking (obs_dim
 *     6 .. 16) the six base entries, not wrapped, the look-ahead entries not read; pendulum the four entries; double pendulum atan2 of
 *     the row's sines and cosines, ONCE.
 *   for t < horizon:  (s_{t+1}, rew_t) = finish(pre(s_t, eps_t), u_t)   on the CARRIED state - the forward sweep's chain, whose processed
 *     rewards mpg_ampc_pg sums.  On the double pendulum this is not the chain of mpg_model_step calls, which reads atan2 of the new row's
 *     sines and cosines again at every step: the two are equal in exact arithmetic, not in bits.
 *   cost = - sum_t rew_t:  RAW rewards (before rew_shift / rew_scale), undiscounted, summed with t ascending.
 * eps [horizon][rows] standard normal in mpg_model_rollout's layout, NULL = zeros: the noise terms at their means (delta_y += 0.5 per
 * step on PathTracking, p += 0.1 on the pendulum; the double pendulum's model has none, eps is not read).  u [rows][horizon][act_dim] are
 * actions in the policy's tanh range; the models apply their own scales (1.2 pi / 9 and 3; 100; 500).
 * mpg_model_mpc_cost_grad, ONE launch, takes u as given (nothing is clamped beyond what the model clamps): cost [rows]; grad (nullable)
 * [rows][horizon][act_dim] = d cost / d u by the chain of the sweeps' hand adjoint of the step from lam_horizon = 0 with rho = -1 -
 * PathTracking's gate on the v_x clamp comes with it (a step whose raw v_x leaves [1, 35] passes no adjoint through v_x); its x (entry
 * 5) is carried for obs_traj and has no adjoint.  obs_traj (nullable) [rows][horizon + 1][obs_dim]: row 0 is obs0's row as given, row
 * t + 1 the observation of s_{t+1} in mpg_model_step's row format (PathTracking's look-ahead entries are copies of delta_y, the double
 * pendulum's eleven features have zeros in 8 .. 10).  rew_traj (nullable) [rows][horizon] RAW.  cost is the same bits whether grad,
 * obs_traj and rew_traj are asked for or not.  float32; the models' own arithmetic (hardware reciprocal / sine / cosine on PathTracking,
 * library sincosf on the pendulums, exact division on the double pendulum), compiled without contraction.
 *
 * mpg_model_mpc_solve, ONE launch: minimises that cost over the box [-1, 1]^(horizon * act_dim) for every row by mpg_mpc_solve's method -
 * the same device loop - with its constants MPG_MPC_SPG_*: spectral projected gradient with the non-monotone line search, the setup
 * u = clamp(u_io, -1, 1), the stop rule max_j |clamp(u - g, -1, 1) - u|_j <= tol (tol 0: never), info = the accepted iterations k, or
 * -(k + 1) behind a failed search.  A NaN (in obs0's row, eps or the start point) fails the first search: info -1, the last accepted
 * point - the clamped start - is kept.  u_io [rows][horizon][act_dim]: start point in, solution out; cost_out [rows] is bit for bit
 * mpg_model_mpc_cost_grad's at the returned u (same eps); pgnorm_out [rows] the norm above at that point.  A row's result does not
 * depend on which other rows share the launch.
 *   INVARIANT: cost_out <= the cost of the clamped start point, for every row.  The cost history starts as [f_0, -inf, ...], so the
 *   first accepted cost is <= f_0 + gamma lambda <g, d> <= f_0 (<g, d> <= 0 for a projected step), and by induction every accepted
 *   cost is below the maximum of costs that are themselves <= f_0.  (A row that accepts nothing keeps f_0.)
 * One lane per row, workgroups of one wave, the lane's arrays in LDS as [index][lane]: per 64 rows (3 act_dim + obs) * horizon + obs
 * floats per lane with obs = 6 / 4 / 6, horizon more for the noise where the model has one, and 25 for the double pendulum's adjoint
 * (102 272 / 64 512 / 79 360 bytes at horizon 31).  Every loop has a fixed bound (iters, the halvings, horizon, the five sub-steps);
 * early exits are wave-uniform.
 * MPG_MODEL_MPC_MAX_ITERS_*: the per-kind bound on iters, the largest round number whose launch at horizon 31 with every CU busy
 * (rows = 64 * the CU count, tol 0) stays under the 0.35 s mpg_mpc_rollout's comment below gives the longest MPC launch on a shared
 * device, and at most MPG_MPC_MAX_ITERS.  Measured on one MI355X, 256 CUs, 16 384 rows, 100 iterations (tools/bench_model_mpc.py --caps):
 * 13.7 / 15.2 / 83.2 ms, the ms per iteration beside each define.
 * Both refuse before any launch with MPG_EINVAL, their own name and a text of its own each, the outputs untouched: a null configuration,
 * an unknown env kind, an obs_dim / act_dim that is not the kind's (6 .. 16 / 2; 4 / 1; 11 / 1), rows <= 0, horizon < 1, horizon >
 * MPG_MPC_MAX_HORIZON, (solve) iters < 0, iters > the kind's MPG_MODEL_MPC_MAX_ITERS_*, a negative or NaN tol, a null pointer other than
 * eps / grad / obs_traj / rew_traj, a tanh output activation with an action range (the cfg no entry point takes).
 * (added without a signature change elsewhere: the ABI version stays 10) */
#define MPG_MODEL_MPC_MAX_ITERS_PATH_TRACKING 1000   /* 0.137 ms per iteration: 2556 fit, MPG_MPC_MAX_ITERS bounds it */
#define MPG_MODEL_MPC_MAX_ITERS_PENDULUM 1000        /* 0.152 ms per iteration: 2307 fit, MPG_MPC_MAX_ITERS bounds it */
#define MPG_MODEL_MPC_MAX_ITERS_DOUBLE_PENDULUM 400  /* 0.832 ms per iteration (five sub-steps, library sincosf, exact division): 420 fit */
int mpg_model_mpc_cost_grad(const mpg_cfg_t* cfg, int rows, int horizon, const float* obs0 /* [rows][obs_dim] */,
                            const float* u /* [rows][horizon][act_dim] */, const float* eps /* nullable, [horizon][rows] */,
                            float* cost /* [rows] */, float* grad /* nullable, [rows][horizon][act_dim] */,
                            float* obs_traj /* nullable, [rows][horizon + 1][obs_dim] */, float* rew_traj /* nullable, [rows][horizon] */,
                            mpg_stream_t stream);
int mpg_model_mpc_solve(const mpg_cfg_t* cfg, int rows, int horizon, int iters, float tol, const float* obs0, const float* eps /* nullable */,
                        float* u_io, float* cost_out, float* pgnorm_out, int* info, mpg_stream_t stream);

/* mpg_model_mpc_rollout, ONE launch: MPC's receding-horizon closed loop ON THE MODEL cfg->env_kind names, for n
 * agents and `steps` model steps with one solve each - mpg_mpc_rollout (below) for the three models of mpg_model_step.  Everything the
 * following chain leaves behind, bit for bit, for t = 0 .. steps - 1:
 *   1. obs_traj[t] = obs_io
 *   2. u = a copy of u_io;  mpg_model_mpc_solve on (cfg, n, horizon, iters, tol, obs_io, eps = NULL, u, cost_traj[t], pgnorm_traj[t],
 *      info_traj[t]) - the planner plans at the noise means;  plan_traj[t] = u
 *   3. warm_start 1: u_io[:, i] = u[:, i + 1] for i < horizon - 1 and u_io[:, horizon - 1] = u[:, horizon - 1] - the plan one action
 *      later, its last action repeated.  warm_start 0: u_io is only read, every solve starts from it.
 *   4. the plant step: mpg_model_mpc_cost_grad on (cfg, n, horizon = 1, obs_io, u[:, 0:1, :], eps ? eps + t * n : NULL, cost = - rew,
 *      grad = NULL, obs_traj', rew_traj[t]);  row 1 of its observation record obs_traj' becomes obs_io.
 * Step 4 is NOT mpg_model_step.  That one's body lives in model_rollout.hip under fp contract(fast) and is kept out of line there because
 * its bits depend on the unit it is compiled in; the solver's model bodies are compiled under contract(off) in model_mpc.hip, and the
 * library is built without relocatable device code: one kernel cannot hold both forms of the model bodies.  The one-step horizon cost is
 * the same model step, in mpg_model_step's row format, under the solver's unit's own rule - and its bits do not depend on which kernel it
 * is inlined into, the property mpg_model_mpc_solve's cost_out already rests on.  The two steps are equal in exact arithmetic and differ
 * by rounding; on the double pendulum both read atan2 of the row's sines and cosines again at every step.
 * eps (nullable) [steps][n] standard normal: the PLANT's model noise (NULL = zeros, the same bits; the double pendulum's model has none,
 * eps is not read).  The planner never sees it.
 * obs_io [n][obs_dim] and (warm) u_io [n][horizon][act_dim] carry everything from one step to the next, so two calls of s1 and s2 steps
 * - eps advanced by s1 * n for the second - equal one call of s1 + s2 steps bit for bit.  Both are written after the LAST step only.
 * From the second step on an observation row is what the step writes: PathTracking's look-ahead entries are copies of delta_y, the
 * double pendulum's entries 8 .. 10 are zeros; obs_traj[0] is the caller's row as given.  obs_traj [steps][n][obs_dim], plan_traj
 * [steps][n][horizon][act_dim] and rew_traj [steps][n] (RAW) are required; cost_traj, pgnorm_traj [steps][n] float and info_traj
 * [steps][n] int are nullable, each on its own.
 * One lane per agent, workgroups of one wave; the lane keeps the entries of its observation row that the model reads (6 / 4 / 8) in
 * registers across the steps, the solver's arrays in LDS as in mpg_model_mpc_solve and of its size, the planner's noise array zeros.
 * Global memory is read in the prologue and then written, never read back - but for u_io with warm_start 0, which no launch of this
 * entry point writes and every solve reads, and eps, one value per lane and step.  An agent's results do not depend on which other
 * agents share the launch.  Every loop has a fixed bound; early exits are wave-uniform.
 * MPG_MODEL_MPC_ROLLOUT_MAX_WORK_* bound steps * iters per kind, the iterations one lane can run in a launch: DERIVED from the
 * per-iteration times above (horizon 31, every CU busy: 0.137 / 0.152 / 0.832 ms) and the 0.35 s mpg_mpc_rollout states as the longest
 * MPC launch on a shared device - 2556 / 2307 / 420 iterations fit under it; 2048 / 2048 / 400 are the round numbers below them.
 * MEASURED for this kernel, one launch at each cap on one MI355X (256 CUs; horizon 31, rows = 64 * the CU count = 16 384, tol 0, cold
 * start; tools/bench_model_mpc.py --caps, the entry point alone between two device events): 16 steps * 128 iterations = 2048 in 0.339 s
 * (PathTracking) and 0.259 s (pendulum), 4 * 100 = 400 in 0.324 s (double pendulum) - all under 0.35 s, no cap was lowered; the times
 * stand beside the defines.  iters stays bounded by the kind's MPG_MODEL_MPC_MAX_ITERS_* as well.  Longer loops run in chunks.
 * WHAT THE BOUND DOES NOT COUNT: every step's solve has a setup forward and reverse pass before its iterations and the plant's step comes
 * on top, about one iteration-equivalent per step that steps * iters leaves out (1 % at 100 iterations per solve).  With few iterations
 * and many steps only MPG_MODEL_MPC_ROLLOUT_MAX_STEPS limits it.  Measured in the same run: PathTracking 1024 steps * 0 / 1 / 2
 * iterations 0.026 / 0.115 / 0.155 s, pendulum 0.021 / 0.133 / 0.169 s - under 0.35 s; double pendulum 1024 * 0: 0.193 s, but 400 * 1:
 * 0.533 s and 200 * 2: 0.382 s - ABOVE it.  A caller on a shared device who runs the double pendulum at one or two iterations per solve
 * keeps steps at 200 or 100.
 * Refuses before any launch with MPG_EINVAL, its own name and a text of its own each, the outputs untouched: what mpg_model_mpc_solve
 * refuses of a configuration, n <= 0, steps < 1, steps > MPG_MODEL_MPC_ROLLOUT_MAX_STEPS, horizon < 1, horizon > MPG_MPC_MAX_HORIZON,
 * iters < 0, iters > the kind's MPG_MODEL_MPC_MAX_ITERS_*, steps * iters > the kind's MPG_MODEL_MPC_ROLLOUT_MAX_WORK_*, a negative or NaN
 * tol, warm_start other than 0 or 1, a null pointer among the required ones, a tanh output activation with an action range.
 * (added without a signature change elsewhere: the ABI version stays 10) */
#define MPG_MODEL_MPC_ROLLOUT_MAX_STEPS 1024
#define MPG_MODEL_MPC_ROLLOUT_MAX_WORK_PATH_TRACKING 2048    /* steps * iters of one launch; 16 * 128 measured at 0.339 s: 2115 fit */
#define MPG_MODEL_MPC_ROLLOUT_MAX_WORK_PENDULUM 2048         /* 16 * 128 measured at 0.259 s: 2764 fit */
#define MPG_MODEL_MPC_ROLLOUT_MAX_WORK_DOUBLE_PENDULUM 400   /* 4 * 100 measured at 0.324 s: 432 fit */
int mpg_model_mpc_rollout(const mpg_cfg_t* cfg, int n, int steps, int horizon, int iters, float tol, int warm_start,
                          float* obs_io /* [n][obs_dim] */, float* u_io /* [n][horizon][act_dim]: the start point of the first solve */,
                          const float* eps /* nullable, [steps][n]: the PLANT's model noise */, float* obs_traj /* [steps][n][obs_dim] */,
                          float* plan_traj /* [steps][n][horizon][act_dim] */, float* rew_traj /* [steps][n] RAW */,
                          float* cost_traj /* nullable */, float* pgnorm_traj /* nullable */, int* info_traj /* nullable */,
                          mpg_stream_t stream);

/* mpg_mpc_rollout, ONE launch: the MPC side of the closed loop of mpc/main.py:168-223 for n agents of PathTracking-v0 with
 * num_future_data = 0 (observations of 6 entries), `steps` env steps with one solve each.  Everything the following chain leaves behind,
 * bit for bit, for t = 0 .. steps - 1:
 *   1. obs_traj[t] = obs_io
 *   2. x0 = obs_io + (20, 0, 0, 0, 0, 0) in float32 (entry 0 becomes (v_x - 20) + 20 from the second step on; the sum with 0 turns a -0
 *      into +0)
 *   3. u = a copy of u_io;  mpg_mpc_solve on (n, horizon, iters, tol, x0, u, cost_traj[t], pgnorm_traj[t], info_traj[t]);  plan_traj[t] = u
 *   4. warm_start 1: u_io[:, i] = u[:, i + 1] for i < horizon - 1 and u_io[:, horizon - 1] = u[:, horizon - 1] - the plan one step later,
 *      its last pair repeated (main.py:214, commented out there).  warm_start 0: u_io is only read, every solve starts from it (:184).
 *   5. mpg_env_step on (MPG_ENV_PATH_TRACKING, n, 6, state, u[:, 0, :], obs_io, rew_traj[t], done_out, done_intended_out)
 * state [MPG_ENV_STATE_DIM][n], obs_io [n][6] and (warm) u_io [n][horizon][2] carry everything from one step to the next, so two calls of
 * s1 and s2 steps equal one call of s1 + s2 steps bit for bit.  They and the two done flags (nullable, uint8 [n]) are written after the
 * LAST step only.  obs_traj [steps][n][6], plan_traj [steps][n][horizon][2] and rew_traj [steps][n] (RAW) are required; cost_traj,
 * pgnorm_traj [steps][n] float and info_traj [steps][n] int are nullable, each on its own.
 * One lane per agent, workgroups of one wave; the agent's state and observation stay in registers across the steps, the solver's arrays
 * in LDS as in mpg_mpc_solve (11 * horizon * 256 bytes per 64 agents).  Global memory is read in the prologue and then written, never
 * read back - but for u_io with warm_start 0, which no launch of this entry point writes and every solve reads.  An agent's results do
 * not depend on which other agents share the launch.
 * MPG_MPC_ROLLOUT_MAX_WORK bounds steps * iters, the iterations one lane can run in a launch, and with it the launch's run time on a
 * shared device: a 200-iteration mpg_mpc_solve at horizon 25 with every CU busy was measured at 33.6 ms, 0.17 ms per iteration, so 2048
 * iterations are about 0.35 s - twice the longest launch mpg_mpc_solve allows (MPG_MPC_MAX_ITERS).  Longer loops are run in chunks.
 * Refuses before any launch with MPG_EINVAL, its own name and a text of its own each, the outputs untouched: n <= 0, steps < 1,
 * steps > MPG_MPC_ROLLOUT_MAX_STEPS, horizon < 1, horizon > MPG_MPC_MAX_HORIZON, iters < 0, iters > MPG_MPC_MAX_ITERS,
 * steps * iters > MPG_MPC_ROLLOUT_MAX_WORK, a negative or NaN tol, warm_start other than 0 or 1, a null pointer among the required ones.
 * (added without a signature change elsewhere: the ABI version stays 10) */
#define MPG_MPC_ROLLOUT_MAX_STEPS 1024
#define MPG_MPC_ROLLOUT_MAX_WORK 2048  /* steps * iters of one launch */
int mpg_mpc_rollout(int n, int steps, int horizon, int iters, float tol, int warm_start,
                    float* state /* [MPG_ENV_STATE_DIM][n], advanced in place */, float* obs_io /* [n][6] */,
                    float* u_io /* [n][horizon][2]: the start point of the first solve */, float* obs_traj /* [steps][n][6] */,
                    float* plan_traj /* [steps][n][horizon][2] */, float* rew_traj /* [steps][n] */, float* cost_traj /* nullable */,
                    float* pgnorm_traj /* nullable */, int* info_traj /* nullable */, uint8_t* done_out /* nullable */,
                    uint8_t* done_intended_out /* nullable */, mpg_stream_t stream);

size_t mpg_mpg_gradients_workspace_bytes(const mpg_cfg_t* cfg, int rows, int M, int n, int n_select, int n_q);
int mpg_mpg_gradients(const mpg_cfg_t* cfg, int n_q, const float* params, const float* target_params, int rows,
                      float* obs, float* act, float* rew, float* obs_tp1, const float* y_in,
                      int M, int n, const int* select, int n_select, const float* w, const float* eps,
                      uint64_t noise_seed, uint64_t noise_ctr, float inv_b_global, float* grad, float* stats,
                      float* y_out, float* sq_part /* nullable: see mpg_sq_partials */,
                      const mpg_replay_draw_t* draw /* nullable */, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* NADPLearner.model_rollout_for_q_estimation  - learners/nadp.py:87-126: from (s, a_replay) roll n model steps,
 * later actions from pi_theta, y = G_n + gamma^n * Q1_target(s~_n, pi_theta(s~_n)) (no gradient).
 * eps [n][rows] standard normal, or NULL for in-kernel Philox(noise_seed, noise_ctr) draws. */
size_t mpg_rollout_q_target_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_rollout_q_target(const mpg_cfg_t* cfg, const float* policy_params, const float* q1t, int rows, int n,
                         const float* obs0, const float* act0, const float* eps, uint64_t noise_seed,
                         uint64_t noise_ctr, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* MPGLearner.model_rollout_for_q_estimation  - learners/mpg_learner.py:180-224 (the heuristic-bias rollout): tile
 * (s, a_replay) M times, roll the model max(select) steps - first action a_replay, later ones from pi_theta - and
 * bootstrap every selected slice k with gamma^k * Q1_target(s~_k, a_k); the InvertedPendulum branch clips that Q to
 * [-0.5, 0] for every slice but the first (:206-209).  y [n_select][rows]: mean over the M copies, slices in the order of
 * `select` (HOST array, n_select <= 4) - the reference's concatenation.  eps [max(select)][M*rows] standard normal, or
 * NULL for in-kernel Philox(noise_seed, noise_ctr) draws.  No gradient. */
size_t mpg_rollout_q_estimation_workspace_bytes(const mpg_cfg_t* cfg, int rows, int M, int n_select);
int mpg_rollout_q_estimation(const mpg_cfg_t* cfg, const float* policy_params, const float* q1t, int rows, int M,
                             const int* select, int n_select, const float* obs0, const float* act0, const float* eps,
                             uint64_t noise_seed, uint64_t noise_ctr, float* y, void* ws, size_t ws_bytes,
                             mpg_stream_t stream);

/* TD3Learner.policy_forward_and_backward  - learners/td3.py:120-134:
 *   loss = -mean_B min(Q1,Q2)(s~, pi(s~)); grad = flat policy gradient (unclipped, reduced over this GPU's rows,
 *   divisor B_global through inv_b_global); qmin_sum / qmin_sqsum: sum and sum of squares of min-Q over the rows
 *   (value_mean / value_var, td3.py:130-132).  The gradient flows through whichever critic is smaller per row. */
size_t mpg_td3_policy_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_td3_policy_grad(const mpg_cfg_t* cfg, const float* policy_params, const float* q1, const float* q2,
                        int rows, const float* obs, float inv_b_global, float* qmin_sum, float* qmin_sqsum,
                        float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* NDPGLearner.policy_forward_and_backward  - learners/ndpg.py:174-186:
 *   loss = -mean_B Q1(s~, pi(s~)); grad = flat policy gradient (unclipped, reduced over this GPU's rows, divisor B_global through
 *   inv_b_global); q_sum / q_sqsum: sum and sum of squares of Q1 over the rows (value_mean / value_var, :180-182).  One critic
 *   forward and one critic backward (mpg_td3_policy_grad runs two of each and refuses a null q2). */
size_t mpg_dpg_policy_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_dpg_policy_grad(const mpg_cfg_t* cfg, const float* policy_params, const float* q1, int rows, const float* obs,
                        float inv_b_global, float* q_sum, float* q_sqsum, float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* ---- SAC with a fixed temperature (learners/sac.py; policy.py:179-204 with action_range None: no bijector) ----
 * The stochastic policy is a diagonal Gaussian over the FOUR logits of the PathTracking policy: mean = logits[:, :2],
 * log_std = clip(logits[:, 2:], -5, 1).  Every entry point below takes the caller's standard-normal draws eps [rows][2]
 * (mpg_normal_fill; no generator runs inside) and refuses, before any launch, with MPG_EINVAL and its own name in the message: null
 * pointers, rows <= 0, act_dim != 2 or env_kind != MPG_ENV_PATH_TRACKING ("Gaussian head without an action range only": the
 * pendulum's action_range 3 is a tanh-affine bijector, policy.py:183-190), action_range > 0, alpha < 0 or not finite; a workspace
 * one byte short is MPG_EWORKSPACE with both sizes.  The queries answer 0 for what the entry points refuse. */

/* PolicyWithQs.compute_action / compute_target_action, stochastic branch  - policy.py:193-217 (act_dist.sample(),
 * act_dist.log_prob):  act_out [rows][2] = mean + sigma * eps, sigma the correctly rounded float32 exp(log_std), product and sum rounded separately,
 * logp_out [rows] = sum_k (-0.5 eps_k^2 - log_std_k - 0.5 log(2 pi)), logits_out [rows][4] (nullable) the policy's output on
 * obs*obs_scale (policy_out_act applied to all four, as MLPNet does). */
size_t mpg_policy_sample_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_policy_sample(const mpg_cfg_t* cfg, const float* policy, int rows, const float* obs, const float* eps, float* act_out,
                      float* logp_out, float* logits_out /* nullable */, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* SACLearner.compute_clipped_double_q_target  - learners/sac.py:67-80:
 *   y = (rew+shift)*scale + gamma * (min(Q1t, Q2t)(s~', a') - alpha * logp'),  (a', logp') sampled from `policy` at s~' with eps
 *   (the reference samples from the ONLINE policy here, sac.py:71: pass the online parameters). */
size_t mpg_sac_targets_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_sac_targets(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                    const float* obs_tp1, const float* eps, float alpha, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* SACLearner.policy_forward_and_backward  - learners/sac.py:119-136:
 *   loss = mean_B (alpha * logp - min(Q1,Q2)(s~, a)),  (a, logp) sampled with eps; grad = flat policy gradient over all four
 *   output columns (unclipped, reduced over this GPU's rows, divisor B_global through inv_b_global).  qmin_sum / qmin_sqsum / logp_sum:
 *   sums over the rows of min-Q, its square and logp (value_mean, value_var, policy_entropy = -mean logp, policy_loss =
 *   alpha * mean logp - value_mean; sac.py:128-132).  A log-std logit outside [-5, 1] has zero gradient (clip_by_value; the
 *   bounds themselves pass it). */
size_t mpg_sac_policy_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_sac_policy_grad(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                        const float* eps, float alpha, float inv_b_global, float* qmin_sum, float* qmin_sqsum, float* logp_sum,
                        float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* ---- SAC with the LEARNED temperature (alpha = 'auto': AlphaModel, its Adam and target_entropy; learners/sac.py:138-148,
 * policy.py:136-143) ----
 * The temperature lives on the device and is read there: no entry point below takes alpha from the host, so a training loop never
 * waits for it.  alpha = exp(log_alpha) is formed as the correctly rounded float32 exponential (the double-precision exp rounded once,
 * the rule of sigma above): np.float32(np.exp(np.float64(log_alpha))) on the host is the same bits.
 *
 * mpg_sac_alpha_t: HOST struct, caller-owned.  state: DEVICE array of 8 floats -
 *   [0] log_alpha   [1] Adam m   [2] Adam v   [3] alpha at the last mpg_sac_alpha_update with do_clip   [4] alpha_loss there
 *   [5] the temperature gradient's norm |g| before the clip   [6] 1.0 where that gradient was not finite, else 0.0   [7] 0
 * lr: PolynomialDecay(lr0, decay_steps, lr_end) of the temperature's own Adam; opt_steps: that Adam's step counter. */
typedef struct {
    float* state;
    float target_entropy;
    float lr[3];
    long long opt_steps;
} mpg_sac_alpha_t;

/* mpg_sac_targets / mpg_sac_policy_grad with const float* log_alpha (device: state + 0) in place of float alpha.  Same workspaces
 * (mpg_sac_targets_workspace_bytes, mpg_sac_policy_grad_workspace_bytes), same refusals under their own names (alpha's excepted),
 * y / grad / qmin_sum / qmin_sqsum / logp_sum bit for bit those of the host-alpha entry points given the same alpha.
 * mpg_sac_policy_grad_auto also evaluates the temperature's loss alpha_loss = mean(-log_alpha (logp_alpha + target_entropy))
 * (sac.py:138-148), logp_alpha the head's log-density under a further draw eps_alpha [rows][2] on the SAME logits (the reference's third
 * compute_action runs the same policy on the same observations: only the noise differs, so there is no third network pass and no
 * further launch):  alpha_grad[0] = -inv_b_global * sum_rows(logp_alpha + target_entropy), this GPU's share of d alpha_loss / d log_alpha
 * (unclipped; shares of unequal shards add up to the full-batch gradient).  The policy gradient does not flow into log_alpha.
 * Refused besides: a target_entropy that is not finite. */
int mpg_sac_targets_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                         const float* obs_tp1, const float* eps, const float* log_alpha, float* y, void* ws, size_t ws_bytes,
                         mpg_stream_t stream);
int mpg_sac_policy_grad_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                             const float* eps, const float* log_alpha, const float* eps_alpha, float target_entropy, float inv_b_global,
                             float* qmin_sum, float* qmin_sqsum, float* logp_sum, float* alpha_grad, float* grad, void* ws,
                             size_t ws_bytes, mpg_stream_t stream);

/* The temperature's scalar step, one small launch.  g: DEVICE, the reduced gradient (the sum of every GPU's alpha_grad).
 * do_clip (SACLearner.compute_gradient): state[3] = alpha, state[4] = alpha_loss = log_alpha * g, state[5] = |g|, state[6] = its
 *   non-finite flag; g[0] = g * clip * min(1 / |g|, 1 / clip) in place (tf.clip_by_global_norm of the one-element list).
 * do_adam (PolicyWithQs.apply_gradients): one Keras-form Adam step on (log_alpha, m, v) - mpg_adam_polyak's arithmetic, the step size
 *   from lr and opt_steps as for the networks - with a ZERO gradient if any of the n_skip_flags device ints is set or state[6] is
 *   (optimizer.py:357-361 zeroes every gradient if any is NaN); opt_steps advances by one either way.
 * Both: the two in that order (the native step's one launch); the same bits as two calls.
 * Refused with MPG_EINVAL, each with its own text: a null struct, a null state, a null g, neither do_clip nor do_adam, clip <= 0 with
 * do_clip, n_skip_flags > 0 behind a null pointer, a negative opt_steps. */
int mpg_sac_alpha_update(mpg_sac_alpha_t* a, float* g, float clip, int do_clip, int do_adam, const int* skip_flags /* nullable */,
                         int n_skip_flags, mpg_stream_t stream);

/* ---- SAC with an action range: the tanh-squashed Gaussian head (policy.py:183-190: the same diagonal Gaussian wrapped in
 * Chain([Affine(scale = action_range), Tanh()]); train_script4mujoco.py built_SAC_parser: InvertedPendulumConti-v0, action_range 3) ----
 * The five entry points above with R = cfg->action_range > 0 and ad = act_dim, u_k = mean_k + sigma_k * eps_k formed as there:
 *   act_k = R * tanh(u_k)
 *   logp  = sum_k (-0.5 eps_k^2 - log_std_k - 0.5 log(2 pi)) - sum_k 2 (log 2 - u_k - softplus(-2 u_k)) - ad * log R
 * (the Tanh bijector's forward_log_det_jacobian and Affine's; evaluated at u itself - TFP's bijector cache hands log_prob the x that
 * produced the sample - not at atanh(act / R)).  logits_out [rows][2 ad] is the policy's plain output: the range never reaches it.
 * The policy gradient of mean(alpha * logp - min Q): dL/du_k = ga_k R (1 - tanh(u_k)^2) + 2 alpha inv_b tanh(u_k), ga the critics'
 * summed input gradient at the action; the mean column receives dL/du_k, the log-std column dL/du_k sigma_k eps_k - alpha inv_b, zero
 * outside [-5, 1].  The _auto forms read alpha = exp(*log_alpha) on the device and sum the SQUASHED log-density under eps_alpha into
 * alpha_grad; given the same alpha they return the fixed-alpha forms' bits.  Same arguments, launches and workspace layouts as the plain
 * siblings (the _auto forms share the fixed-alpha queries); eps / eps_alpha are [rows][act_dim].
 * Served: act_dim 2 on MPG_ENV_PATH_TRACKING with obs_dim 6 .. 16, and act_dim 1 with obs_dim 4 on MPG_ENV_INVERTED_PENDULUM.
 * Refused before any launch with MPG_EINVAL, each with its own text under the entry point's name, prefilled outputs untouched: null
 * pointers (logits_out alone may be null), rows <= 0, MPG_ENV_INVERTED_DOUBLE_PENDULUM, another act_dim / env_kind pair,
 * action_range <= 0 or not finite, policy_out_act MPG_ACT_TANH together with the range, another observation width, alpha < 0 or not
 * finite, a target_entropy that is not finite; a workspace one byte short is MPG_EWORKSPACE with both sizes.  The queries answer 0 for
 * what the entry points refuse.  The plain entry points keep refusing every cfg with a range. */
size_t mpg_policy_sample_squashed_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_policy_sample_squashed(const mpg_cfg_t* cfg, const float* policy, int rows, const float* obs, const float* eps, float* act_out,
                               float* logp_out, float* logits_out /* nullable */, void* ws, size_t ws_bytes, mpg_stream_t stream);
size_t mpg_sac_targets_squashed_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_sac_targets_squashed(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                             const float* obs_tp1, const float* eps, float alpha, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream);
size_t mpg_sac_policy_grad_squashed_workspace_bytes(const mpg_cfg_t* cfg, int rows);
int mpg_sac_policy_grad_squashed(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                                 const float* eps, float alpha, float inv_b_global, float* qmin_sum, float* qmin_sqsum, float* logp_sum,
                                 float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream);
int mpg_sac_targets_squashed_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                                  const float* obs_tp1, const float* eps, const float* log_alpha, float* y, void* ws, size_t ws_bytes,
                                  mpg_stream_t stream);
int mpg_sac_policy_grad_squashed_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows,
                                      const float* obs, const float* eps, const float* log_alpha, const float* eps_alpha,
                                      float target_entropy, float inv_b_global, float* qmin_sum, float* qmin_sqsum, float* logp_sum,
                                      float* alpha_grad, float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * clip_by_global_norm + Keras Adam + Polyak (K7, K8) over the flat [net0 | net1 | ...] vectors
 * ---------------------------------------------------------------------------------------------- */

/* tf.clip_by_global_norm(g, clip) applied to each of the n_seg (<= 8) consecutive networks of `grad`
 * (seg_sizes: HOST array of their lengths) - learners/mpg_learner.py:415-431: norms[k] = ||g_k||_2,
 * g_k *= clip * min(1/norm, 1/clip) in place.  nonfinite_flags (device int[n_seg], nullable) receives 1 for
 * every network whose norm is not finite, else 0 (optimizer.py:357-361 zeroes such gradient lists).  Must run
 * AFTER the cross-GPU all-reduce: the clip is not linear. */
#define MPG_CLIP_PARTS 272 /* partial sums of squares per network: one per 256 elements up to 69 632, strided beyond */
int mpg_clip_by_global_norm(float* grad, const int* seg_sizes, int n_seg, float clip, float* norms,
                            int* nonfinite_flags,
                            float* scratch /* nullable: n_seg*MPG_CLIP_PARTS floats -> parallel two-launch form */,
                            mpg_stream_t stream);

/* The first half of the parallel clip on its own: sq_part[k*MPG_CLIP_PARTS + b] = sum of squares of block b
 * (elements 256 b ... 256 b + 255, + multiples of 256*MPG_CLIP_PARTS) of network k, fixed summation order. */
int mpg_sq_partials(const float* grad, const int* seg_sizes, int n_seg, float* sq_part, mpg_stream_t stream);

/* mpg_clip_by_global_norm's second half + mpg_adam_polyak in ONE launch: norms from sq_part (mpg_sq_partials or
 * mpg_mpg_gradients' by-product), grad scaled in place (it is the list compute_gradient returns), NaN guard
 * (optimizer.py:357-361: any non-finite norm -> every Adam step sees zeros), Adam, Polyak.  Bit-identical to
 * mpg_clip_by_global_norm(scratch) followed by mpg_adam_polyak(skip_flags = nonfinite_flags). */
int mpg_clip_adam_polyak(float* w, float* m, float* v, float* target, float* grad, const float* sq_part,
                         const int* seg_sizes, int n_seg, float clip, const float* lr_t, const int* do_adam,
                         const int* do_polyak, float tau, float* norms, int* nonfinite_flags,
                         const mpg_wcache_t* wc_w /* nullable: packed images of w, kept current */,
                         const mpg_wcache_t* wc_target /* nullable: same for target */, mpg_stream_t stream);

/* PolicyWithQs.apply_gradients + update_*_target  - policy.py:123-171.  For every network k (HOST arrays):
 * do_adam[k]: one Keras Adam step (beta .9/.999, eps 1e-7 outside the sqrt, TF ApplyAdam form) with the
 * bias-corrected rate lr_t[k] = lr(step)*sqrt(1-b2^t)/(1-b1^t) computed by the caller from ITS per-optimizer
 * step counter and PolynomialDecay schedule (policy.py:54-70); do_polyak[k]: target = tau*w + (1-tau)*target
 * afterwards.  If any of skip_flags[0..n_skip_flags) (device ints, nullable) is non-zero the gradient is taken as
 * zeros (NaN guard, optimizer.py:357-361). */
int mpg_adam_polyak(float* w, float* m, float* v, float* target, const float* grad, const int* seg_sizes,
                    int n_seg, const float* lr_t, const int* do_adam, const int* do_polyak, float tau,
                    const int* skip_flags, int n_skip_flags,
                    const mpg_wcache_t* wc_w /* nullable: packed images of w, kept current */,
                    const mpg_wcache_t* wc_target /* nullable: same for target */, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * On-device replay ring (K9, uniform part)  - buffer.py:21-91
 * ---------------------------------------------------------------------------------------------- */

/* ReplayBuffer.add_batch (buffer.py:46-55,80-82): writes n transitions at ring positions
 * (next_idx + i) % capacity.  Ring arrays: obs [cap][obs_dim], act [cap][act_dim], rew [cap],
 * obs2 [cap][obs_dim], done [cap] bytes - RAW observations and rewards. */
int mpg_replay_add(int capacity, int next_idx, int n, int obs_dim, int act_dim, const float* s_obs,
                   const float* s_act, const float* s_rew, const float* s_obs2, const uint8_t* s_done,
                   float* obs, float* act, float* rew, float* obs2, uint8_t* done, mpg_stream_t stream);

/* ReplayBuffer._encode_sample (buffer.py:57-68): gathers rows idx[i] of the ring; o_done (nullable) is
 * written as float32 like the learners' cast (mpg_learner.py:71). */
int mpg_replay_gather(int n, const int* idx, int obs_dim, int act_dim, const float* obs, const float* act,
                      const float* rew, const float* obs2, const uint8_t* done, float* o_obs, float* o_act,
                      float* o_rew, float* o_obs2, float* o_done, mpg_stream_t stream);

/* ReplayBuffer.sample (buffer.py:70-78) in one launch: mpg_uniform_indices + mpg_replay_gather (same Philox stream,
 * same results). */
int mpg_replay_sample_uniform(int n_storage, int n, uint64_t seed, uint64_t ctr, int obs_dim, int act_dim,
                              const float* obs, const float* act, const float* rew, const float* obs2,
                              const uint8_t* done, int* idx, float* o_obs, float* o_act, float* o_rew, float* o_obs2,
                              float* o_done, mpg_stream_t stream);

/* ReplayBuffer.sample_idxes (buffer.py:70-71): n indices uniform in [0, n_storage), with replacement,
 * from Philox(seed, ctr). */
int mpg_uniform_indices(int n_storage, int n, uint64_t seed, uint64_t ctr, int* idx, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * On-device prioritized replay (K9, proportional part)  - buffer.py:94-189, utils/segment_tree.py:13-151
 * ---------------------------------------------------------------------------------------------- */

/* Each tree is ONE float64 array of 2*capacity nodes in the reference's heap order (node 1 = root, leaves at
 * [capacity, 2*capacity), capacity a power of two, segment_tree.py:40-44); float64 because the reference keeps
 * python floats.  stamp: int scratch [capacity] owned by the caller (duplicate-index resolution). */

/* SegmentTree.__init__: neutral elements 0.0 / +inf (segment_tree.py:106,146); stamp = -1. */
int mpg_per_init(double* sum_tree, double* min_tree, int* stamp, int capacity, mpg_stream_t stream);

/* Batched SegmentTree.__setitem__ (segment_tree.py:90-97) = PrioritizedReplayBuffer.update_priorities / add
 * (buffer.py:127-136,166-189): leaf[idx[i]] = (|prio[i]| + eps)^alpha in both trees (the reference asserts
 * priority > 0; learners hand signed td errors, SURVEY.md B-3, hence |.| + eps), then every internal node is
 * recomputed as left + right / min(left, right).  Duplicates: the last entry of the batch wins, like the
 * reference's sequential loop.  max_priority (device DOUBLE since ABI 10 - the reference's _max_priority is a python float -,
 * nullable) tracks max(|prio| + eps) over every entry of the batch, overridden duplicates included (buffer.py:182-189: one max()
 * per entry of the sequential loop). */
int mpg_per_update(double* sum_tree, double* min_tree, int* stamp, int capacity, int n, const int* idx,
                   const float* prio, double alpha, double eps, double* max_priority, mpg_stream_t stream);

/* PrioritizedReplayBuffer.add for n consecutive ring slots start, start + 1, ... (mod ring_capacity): their leaves enter at the
 * current max priority, (*max_priority) ** alpha in float64 (buffer.py:127-136).  idx_scratch: n ints of device scratch. */
int mpg_per_add(double* sum_tree, double* min_tree, int* stamp, int capacity, int ring_capacity, int start, int n,
                double alpha, double* max_priority, int* idx_scratch, mpg_stream_t stream);

/* PrioritizedReplayBuffer._sample_proportional + IS weights (buffer.py:138-160):
 *   mass_i = u_i * sum(0, n_storage)  (inclusive end, buffer.py:141);  idx_i = find_prefixsum_idx(mass_i)
 *   (segment_tree.py:114-140);  w_i = (p_i/sum * n_storage)^-beta / max_w  with max_w from the min tree.
 * u [n] uniform(0,1) float64 draws supplied by the caller (NULL: 53-bit Philox(seed, ctr) draws). */
int mpg_per_sample(const double* sum_tree, const double* min_tree, int capacity, int n_storage, int n,
                   const double* u, uint64_t seed, uint64_t ctr, double beta, int* idx, float* is_weight,
                   mpg_stream_t stream);
/* The same draw with the gather of the sampled transitions in the same launch: PrioritizedReplayBuffer.sample, buffer.py:161-164
 * (_sample_proportional + IS weights + _encode_sample).  Results identical to mpg_per_sample followed by mpg_replay_gather.
 * o_done (nullable): the dones as float, like mpg_replay_gather. */
int mpg_per_sample_gather(const double* sum_tree, const double* min_tree, int capacity, int n_storage, int n,
                          const double* u, uint64_t seed, uint64_t ctr, double beta, int* idx, float* is_weight,
                          int obs_dim, int act_dim, const float* ring_obs, const float* ring_act, const float* ring_rew,
                          const float* ring_obs2, const uint8_t* ring_done, float* o_obs, float* o_act, float* o_rew,
                          float* o_obs2, float* o_done, mpg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Native step driver  - SingleProcessOffPolicyOptimizer.step, optimizer.py:330-362
 * ---------------------------------------------------------------------------------------------- */

/* One training iteration of the MPG learner (round 4: also NADP and TD3 + prioritized replay) enqueued by native code, so that the ~45 kernel launches of a step are
 * not paced by the Python interpreter.  It calls exactly the entry points above, in the reference's order:
 *   mpg_step_begin:  [every sampling_interval-th iteration: sample_iters x (policy + N(0,sigma) -> env.step ->
 *                    ring add -> env.reset)]  (worker.py:91-119, optimizer.py:332-337);  replay (uniform indices +
 *                    gather, buffer.py:70-91);  target (MPG-v2: mpg_learner.py:126-134; MPG-v1: 25 real-env steps +
 *                    n-step return, :146-169);  Q loss/gradients (:326-354);  model rollout + mixed policy gradient
 *                    (:226-286,356-365).  Leaves UN-clipped partials scaled by 1/(batch*world_size) in grad[].
 *   (the caller all-reduces grad[0 .. n_grad+16) across GPUs here)
 *   mpg_step_end:    per-network clip_by_global_norm (:415-431) + Adam/Polyak (policy.py:123-171).
 * All pointers are device buffers owned by the caller; counters are advanced in place (host fields). */
typedef struct {
    mpg_cfg_t cfg;
    int learner_version;              /* 1: MPG-v1 (n-step real-env target; on the pendulum, env_kind 1, with the bootstrap value
                                            clipped to [MPG_PENDULUM_NSTEP_Q_LO, _HI]: mpg_nstep_targets_clipped), 2: MPG-v2 (clipped double-Q target),
                                         3: NADP (learners/nadp.py:209-241: networks [Q1 | policy]; n = the Q-target AND policy
                                            rollout horizon, n_select / select / eta / total_ite unused),
                                         4: TD3 (learners/td3.py:150-188: networks [Q1 | Q2 | policy]; n, M, select unused),
                                         5: NDPG (learners/ndpg.py:202-237: networks [Q1 | policy]; n = sample_num_in_learner, the
                                            real-env n-step target of version 1 (mpg_env_rollout into l_rewards / l_obs) every
                                            num_batch_reuse-th call; M, n_select / select / eta / total_ite unused),
                                         7: SAC, fixed temperature (learners/sac.py:169-219: networks [Q1 | Q2 | policy], uniform
                                            replay; n, M, select, smooth_* unused).  Served by mpg_sac_step_begin, which carries the
                                            temperature as an argument (this struct gains no field: the ABI version stays 10);
                                            mpg_step_begin refuses it and names that function.  6 is not assigned: it stays refused
                                            everywhere (mpg_step_workspace_bytes, mpg_step_begin, mpg_sac_step_begin),
                                         8: AMPC (learners/ampc.py:105-122: networks [policy] alone, uniform replay, a fresh batch on
                                            every call: num_batch_reuse must be 1; n = the rollout horizon, 0 < n < 32, M copies per row,
                                            batch * M % 16 == 0.  The two statistics - the sums of the M-mean reward sum and of its
                                            square - are grad[n_grad] and grad[n_grad + 1].  n_select / select / eta / total_ite, ws0 /
                                            ws0_bytes, b_targets, tau and delay_update are not read: a policy-only stack has no delay
                                            and no target (policy.py:125-127).  `targets` stays a required pointer - mpg_step_end's
                                            launch and the weight-cache pair take it - and is never written.  Served by
                                            mpg_step_workspace_bytes, mpg_step_begin and mpg_step_end: no new symbol, no new field, the
                                            ABI version stays 10.  mpg_sac_step_begin / mpg_sac_auto_step_* refuse it */
    int num_agent, sample_iters;      /* worker: sample_iters env steps of num_agent agents per sampling call.  mpg_step_begin issues
                                         all of them but the one that pre-gathers MPG-v2's draw as ONE launch (mpg_worker_rollout,
                                         bit-identical) where there are at least two, the ring holds them (iters * num_agent <=
                                         ring_capacity) and the width's measurement says so (obs_dim 6), else one
                                         mpg_worker_step each.  On the pendulum's real env (env_kind 1, obs_dim 4, act_dim 1) all of
                                         them are ONE mpg_worker_rollout_pendulum under the same two conditions, else
                                         mpg_policy_action + mpg_env_step_store_reset each.  sample_iters < 0 (one more accepted value of this int: no layout
                                         changed) asks for |sample_iters| steps with the chain KEPT: the A/B form of that measurement.
                                         Version 7 (mpg_sac_step_begin / mpg_sac_auto_step_begin): all of them are ONE
                                         mpg_worker_sample_rollout under the same two conditions, at every obs_dim, else
                                         one mpg_worker_sample_step each; sample_iters < 0 keeps that chain likewise.
                                         Version 1 on the pendulum: the learner's n real-env steps behind the n-step target are ONE
                                         mpg_env_rollout_pendulum for n <= 1024; sample_iters < 0 keeps that chain
                                         too (mpg_env_reset_from_obs, then mpg_policy_action + mpg_env_step per step) */
    int sampling_interval;            /* optimizer.py:331 (10 in the reference) */
    int batch, n, M, n_select, select[4];
    float eta;                        /* rule_based_weights, mpg_learner.py:384-399 */
    int total_ite;
    float clip, tau;
    int delay_update, num_batch_reuse, world_size;
    int grads_exchanged;              /* != 0: the caller sums grad[] across processes between mpg_step_begin and mpg_step_end
                                         (every run with world_size > 1): the clip's partial sums of squares are then taken
                                         from the exchanged gradient in mpg_step_end instead of being a by-product of
                                         mpg_step_begin's last launch.  Same partials, same order, either way. */
    float explore_sigma;
    float value_lr[3], policy_lr[3];  /* PolynomialDecay(lr0, steps, lr_end), policy.py:54-70 */
    /* counters */
    uint64_t worker_seed, noise_ctr, env_seed, env_ctr, replay_seed, replay_times, learner_seed, learner_counter;
    int ring_capacity, ring_next, ring_size;
    long long opt_steps[3];           /* per-optimizer step counters in network order Q1,(Q2),policy */
    /* worker / env */
    float *env_state, *w_obs, *w_act, *w_rew, *w_obs2;
    uint8_t *w_done, *w_done_intended;
    /* replay ring and the sampled minibatch */
    float *ring_obs, *ring_act, *ring_rew, *ring_obs2;
    uint8_t* ring_done;
    int* idx;
    float *b_obs, *b_act, *b_rew, *b_obs2, *b_done, *b_targets;
    /* networks [Q1 | (Q2) | policy], their targets, Adam moments */
    float *params, *targets, *adam_m, *adam_v;
    float* grad;                      /* n_grad + 16 floats: gradients then statistics (q losses, return sums) */
    float* norms;                     /* n_nets */
    float* clip_scratch;              /* n_nets * MPG_CLIP_PARTS floats */
    int* nonfinite;                   /* n_nets */
    /* MPG-v1: the learner's own env for the n-step sampler (batch agents).  NDPG (5): l_rewards [n][batch] and l_obs only */
    float *l_env_state, *l_obs, *l_act, *l_rewards;
    uint8_t *l_done, *l_done_intended;
    void *ws0, *ws1;
    size_t ws0_bytes, ws1_bytes;
    /* TD3 (learner_version 4) */
    float smooth_sigma, smooth_clip;  /* target policy smoothing, td3.py:74-76 (noise: mpg_normal_fill(learner_seed, learner_counter)) */
    int prioritized;                  /* != 0: PrioritizedReplayBuffer (buffer.py:94-189) - the fields below; 0: uniform replay */
    double *per_sum, *per_min;        /* segment trees, 2 * per_capacity doubles each (mpg_per_init) */
    int* per_stamp;
    int per_capacity;
    double* per_max_priority;         /* float64 (ABI 10): the reference's _max_priority is a python float */
    double per_alpha, per_beta, per_eps;
    float* b_weights;                 /* [batch] IS weights of the draw (buffer.py:146-160; the TD3 loss does not use them) */
    float* scratch;                   /* max(batch * (act_dim + 3), 2 * num_agent) floats: smoothing noise | y1 | td | priority errors
                                         (and the index / priority pairs of a ring add).
                                         SAC (learner_version 7): max(batch * act_dim, num_agent * (act_dim + 1)) floats - the
                                         learner's draws [batch][act_dim]; the second size is room for a worker's draws
                                         [num_agent][act_dim] and log-densities [num_agent], which the one-launch worker step
                                         the driver takes (mpg_worker_sample_step) forms in registers and does not store.
                                         With the learned temperature (mpg_sac_auto_step_begin): max(2 * batch * act_dim, that) - the
                                         draw of the temperature's loss [batch][act_dim] behind the learner's */
    /* scheduling option (round 5, ABI 9; MPG only, optional) */
    void* critics_ready_event;        /* hipEvent_t, nullable: see mpg_grad_opts_t (the caller overlaps the critics' exchange) */
    mpg_grad_opts_t grad_opts;        /* storage for cfg.grad_opts during mpg_step_begin */
    /* round 6, ABI 10 */
    int clip_partials_ready;          /* != 0 (meaningful with grads_exchanged): the caller's exchange left the clip partials of the
                                         REDUCED gradient in clip_scratch (mpg_sum_slots_sq) - mpg_step_end takes them as given
                                         instead of re-reading grad[] (mpg_sq_partials).  `grad` may differ between mpg_step_begin
                                         (where the partial gradient is written: e.g. the caller's own staging slot of the
                                         exchange) and mpg_step_end (the reduced buffer): it is read at call time. */
} mpg_train_ctx_t;

/* learner_version 8 - SingleProcessOffPolicyOptimizer.step with AMPCLearner.compute_gradient (ampc.py:105-122), the calls in order:
 *   mpg_step_begin:  [every sampling_interval-th iteration: the worker's sample as for version 3 - the one-launch samples
 *                    (mpg_worker_rollout / mpg_worker_rollout_pendulum) where sample_iters says so, the chain with sample_iters < 0,
 *                    explore_sigma passed on; noise_ctr, env_ctr, ring_next, ring_size advance per iteration];  replay_times++;
 *                    mpg_replay_sample_uniform;  learner_counter++;  mpg_ampc_pg(cfg, policy, batch, M, n, b_obs, eps = NULL,
 *                    learner_seed, 2 * learner_counter + 1, 1 / (batch * world_size), grad + n_grad, grad + n_grad + 1, grad, ws1).
 *   mpg_step_end:    mpg_sq_partials as for every non-MPG version (clip_partials_ready stands after an exchange), then
 *                    mpg_clip_adam_polyak over the one segment with the policy's learning rate, do_adam = 1 on EVERY iteration and
 *                    do_polyak = 0 always; opt_steps[0] advances on every call.  delay_update and tau are not looked at.
 *   mpg_step_workspace_bytes: *ws0 = 0, *ws1 = mpg_ampc_pg_workspace_bytes(cfg, batch, M, n).
 * Refused by mpg_step_begin with MPG_EINVAL, its name and a text of its own each, before anything is enqueued or any counter moves
 * (what mpg_ampc_pg would refuse is found through its workspace query up front, not after the sample has run): n outside 0 < n < 32,
 * batch * M % 16 != 0, M <= 0, an unsupported cfg (the workspace query refuses these four under its own name), num_batch_reuse != 1,
 * prioritized != 0, env_kind 2 (the text of every version), a null pointer among params, targets, grad, ws1, env_state, w_obs, w_act,
 * w_done, ring_*, idx, b_obs, b_act, b_rew, b_obs2, b_done (named in the text); ws1_bytes below the need: MPG_EWORKSPACE with both sizes. */

/* workspace requirements of a context (ws0: targets / critic; ws1: rollout) */
int mpg_step_workspace_bytes(const mpg_train_ctx_t* ctx, size_t* ws0_bytes, size_t* ws1_bytes);
int mpg_step_begin(mpg_train_ctx_t* ctx, int iteration, mpg_stream_t stream);
int mpg_step_end(mpg_train_ctx_t* ctx, int iteration, mpg_stream_t stream);

/* mpg_step_begin for learner_version 7 - SingleProcessOffPolicyOptimizer.step with SACLearner.compute_gradient (sac.py:169-219) on a
 * uniform replay ring, through the entry points above only and with the counters advanced as the Python classes advance them:
 *   [every sampling_interval-th iteration, sample_iters x: the stochastic worker step keyed by (worker_seed, noise_ctr++) and
 *    (env_seed, env_ctr++) -> ring - as ONE mpg_worker_sample_rollout where mpg_train_ctx_t.sample_iters says so, bit-identical];  replay_times++;  on every num_batch_reuse-th call: mpg_replay_sample_uniform,
 *   mpg_normal_fill(batch * act_dim, learner_seed, 2 * (learner_counter + 1)), mpg_sac_targets with the ONLINE policy and both target
 *   critics into b_targets;  learner_counter++;  mpg_q_loss_grad for Q1 and Q2 (statistics 0, 1);
 *   mpg_normal_fill(batch * act_dim, learner_seed, 2 * learner_counter + 1);  mpg_sac_policy_grad (statistics 2 .. 4: the sums of
 *   min-Q, its square and logp).  Gradients are scaled by 1 / (batch * world_size).  mpg_step_end follows as for every version.
 * ws0 / ws1: mpg_step_workspace_bytes (ws0: the larger of the mpg_sac_targets and mpg_q_loss_grad workspaces; ws1:
 * mpg_sac_policy_grad's).  Refused with MPG_EINVAL before anything is enqueued: a learner_version other than 7, an incomplete context
 * (scratch included), prioritized != 0, explore_sigma != 0, alpha negative or not finite, env_kind 2. */
int mpg_sac_step_begin(mpg_train_ctx_t* ctx, float alpha, int iteration, mpg_stream_t stream);

/* The same step with the LEARNED temperature (mpg_sac_alpha_t above; SACLearner with alpha = 'auto').
 * mpg_sac_auto_step_begin: mpg_sac_step_begin with mpg_sac_targets_auto / mpg_sac_policy_grad_auto on a->state (alpha is read on the
 *   device) and a->target_entropy, and one more draw for the temperature's loss, mpg_normal_fill(batch * act_dim, learner_seed + 2,
 *   learner_counter) after the counter's increment, into scratch + batch * act_dim.  The gradient buffer is
 *   [grads | the temperature's gradient | statistics]: grad[n_grad] is this GPU's share, the statistics start at grad + n_grad + 1, and
 *   the ONE exchange covers them all.  Refusals: those of mpg_sac_step_begin (alpha's excepted) under this name, a null struct, a null
 *   state, a target_entropy that is not finite - each with its own text, before anything is enqueued or counted.
 * mpg_sac_auto_step_end: mpg_step_end, then mpg_sac_alpha_update(a, grad + n_grad, ctx->clip, do_clip = 1,
 *   do_adam = (iteration % delay_update == 0), ctx->nonfinite, n_nets): one more launch; a->opt_steps advances with the policy's.
 *   Refusals: a null context, a learner_version other than 7, a null struct, a null state, an incomplete context. */
int mpg_sac_auto_step_begin(mpg_train_ctx_t* ctx, const mpg_sac_alpha_t* a, int iteration, mpg_stream_t stream);
int mpg_sac_auto_step_end(mpg_train_ctx_t* ctx, mpg_sac_alpha_t* a, int iteration, mpg_stream_t stream);

/* The lagged worker sample - the reference's default optimizer, OffPolicyAsync, whose workers sample with weights up to
 * max_weight_sync_delay iterations old and whose rows arrive when they arrive, in a DETERMINISTIC form.  With lag = L
 * (1 <= L <= sampling_interval) the sample that starts at iteration k (k % sampling_interval == 0) reads the policy as it stands at
 * the start of iteration k; its rows enter the ring (and the priority trees) at the start of iteration k + L, before that iteration's
 * draw; the draws of iterations k .. k + L - 1 do not see them.  noise_ctr and env_ctr advance at k; ring_next, ring_size and the
 * trees at k + L.  The sample's launches then need nothing the step writes, and run on a second stream beside it.
 *
 * The object is the caller's, like mpg_prof_t: the library keeps nothing.  Every pointer is a device buffer of the caller; the stream
 * and the two events are created by the caller ONCE (nothing is created inside a step) and outlive the last call.
 *   pending, due: host-side state, zero before the first call; the library counts the iterations staged and the iteration they are
 *   due at.  lag <= sampling_interval keeps it to one pending sample. */
typedef struct {
    int lag;                 /* 1 .. ctx->sampling_interval */
    mpg_stream_t side;       /* hipStream_t of the sample's launches.  NULL, or the step's own stream: no event is touched and the same
                                calls run in the same order on the one stream - the reference form (bit-identical) */
    void *forked, *done;     /* hipEvent_t, required with a side stream: `forked` is recorded on the step's stream where the sample may
                                start, `done` on the side stream behind the sample's last launch */
    float* policy;           /* the worker's copy of the policy network: net_size(obs_dim, 2 * act_dim) floats.  It lies outside every
                                mpg_wcache_t, so the sample's launches take the strided weight loads (bit-identical; packed images of
                                the copy measured no faster: DESIGN.md 7 f18) */
    float *s_obs, *s_act, *s_rew, *s_obs2;   /* staging rows of ONE sample, laid out as the ring: |sample_iters| * num_agent rows */
    uint8_t* s_done;
    int pending;             /* iterations staged and not yet added (0: none) */
    int due;                 /* the iteration at whose start they are added */
} mpg_lagged_sample_t;

/* mpg_step_begin / mpg_sac_step_begin / mpg_sac_auto_step_begin with a lagged sample; mpg_step_end / mpg_sac_auto_step_end follow as
 * they are.  No field of mpg_train_ctx_t and no existing signature changed: the ABI version stays 10.  The calls, in order:
 *   1. a sample is due (pending and iteration >= due): the step's stream waits for `done`; mpg_replay_add(ring_capacity, ring_next,
 *      pending * num_agent rows) from the staging rows, wrap included; on a prioritized context one mpg_per_add per iteration, in
 *      iteration order; ring_next and ring_size advance.  All on the step's stream, before the draw.
 *   2. iteration % sampling_interval == 0: the policy's floats are copied into `policy` ON THE STEP'S STREAM (this iteration's
 *      mpg_step_end writes them; a copy on the side stream would race it); `forked` is recorded there - behind the last optimizer launch
 *      and behind the add of 1., which is what makes the staging rows free again - and the side stream waits for it;
 *      the sample's launches run on the side stream exactly as mpg_step_begin would issue them (the one-launch sample or the chain:
 *      sample_iters as documented above) with the staging rows as their ring - capacity = the rows of one sample, position 0, then
 *      it * num_agent along a chain - reading `policy`, the env state, w_* and the status word (OR-ed atomically by both streams) and
 *      nothing the step writes before the join; `done` is recorded.  MPG-v2's pre-gathered draw is not taken: it exists because the draw
 *      follows the add.  noise_ctr, env_ctr advance; pending = |sample_iters|, due = iteration + lag.
 *   3. replay_times++ and the version's gradients, unchanged.
 * w_obs, w_done and the env state belong to the side stream from the fork to the next join (or drain).
 * Refused with MPG_EINVAL under the entry point's name, before anything is enqueued or counted: a null object; everything the plain
 * begin of the version refuses; lag outside 1 .. sampling_interval; missing staging rows; a missing policy copy; cfg.prof together
 * with a side stream (its events belong to one stream); a side stream without both events; world_size > 1; sample_iters == 0; a ring
 * smaller than one sample; an empty ring with nothing due; a sample still pending at a sampling iteration.
 * mpg_lagged_sample_drain: a pending sample is joined and added now (step 1 alone), whatever its due iteration - the end of a run,
 * or ahead of anything that reads the ring, the worker's observation or the env state on the host side. */
int mpg_step_begin_lagged(mpg_train_ctx_t* ctx, mpg_lagged_sample_t* lagged, int iteration, mpg_stream_t stream);
int mpg_sac_step_begin_lagged(mpg_train_ctx_t* ctx, float alpha, mpg_lagged_sample_t* lagged, int iteration, mpg_stream_t stream);
int mpg_sac_auto_step_begin_lagged(mpg_train_ctx_t* ctx, const mpg_sac_alpha_t* a, mpg_lagged_sample_t* lagged, int iteration,
                                   mpg_stream_t stream);
int mpg_lagged_sample_drain(mpg_train_ctx_t* ctx, mpg_lagged_sample_t* lagged, mpg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPG_HIP_H */
