// Native step driver: SingleProcessOffPolicyOptimizer.step (optimizer.py:330-362), built purely from the public entry points of this
// library so that Python is not on the launch path.  One table describes the learner versions (VERSIONS), one function is the worker's
// sample (sample), one skeleton stands behind the three begin entry points (begin); what a version enqueues is its *_gradients
// function, read top to bottom.  The lagged worker sample (mpg_lagged_sample_t: the *_lagged entry points at the end) is the same sample and
// the same gradients with the add moved `lag` iterations on, so that the sample can run on a second stream beside the steps between.
#include <algorithm>
#include <cmath>

#include "adam_schedule.h"
#include "mpg_common.h"

namespace {

constexpr int H = MPG_HIDDEN;
inline int net_size(int in_dim, int out_dim) { return in_dim * H + H + H * H + H + H * out_dim + out_dim; }

#define TRY(call)            \
    do {                     \
        int rc_ = (call);    \
        if (rc_) return rc_; \
    } while (0)

#define HIP_TRY(entry, call)                                                   \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            mpg_set_error("%s: %s: %s", entry, #call, hipGetErrorString(e_));  \
            return -(int)e_;                                                   \
        }                                                                      \
    } while (0)

struct Layout {
    int n_nets, q_size, p_size, n_grad;
    int sizes[3], off[3];   // Q1, (Q2), policy
};

// what one begin call hands its version's gradient function
struct Step {
    int iteration;
    bool fresh;                  // this call draws a new minibatch: every num_batch_reuse-th does (mpg_learner.py:402-403, ndpg.py:203-204)
    int predrawn_at;             // >= 0: the worker's last launch has gathered the draw but for the ring rows it was writing, from here on
    float alpha;                 // SAC: the fixed temperature, or
    const mpg_sac_alpha_t* at;   //      (non-null) the learned one, read on the device
};

enum Version { MPG_V1 = 1, MPG_V2 = 2, NADP = 3, TD3 = 4, NDPG = 5, SAC = 7, AMPC = 8 };

struct Traits {
    int n_critics;         // the networks are [Q1 | (Q2) | policy]; without a critic there is no ws0
    bool target;           // target networks: Polyak, and the policy's delayed update (a policy-only stack has neither, policy.py:125-127)
    bool batch_reuse;      // num_batch_reuse > 1 is served
    bool prioritized;      // a prioritized replay is served: the worker's transitions enter the trees
    bool stochastic;       // the worker samples its action from the policy's Gaussian head
    bool predraw;          // the minibatch is drawn right after the add: the worker's last launch may gather it
    bool clip_partials;    // the gradient launch leaves the clip's partial sums of squares behind
    bool (*complete)(const mpg_train_ctx_t*);                           // the fields and pointers of its own that it requires
    void (*workspace)(const mpg_train_ctx_t*, size_t* ws0, size_t* ws1);
    int (*gradients)(mpg_train_ctx_t*, const Layout&, const Step&, mpg_stream_t);
};
const Traits* traits(int version);      // null for a version that is not assigned

inline bool exchanged(const mpg_train_ctx_t* c) { return c->world_size > 1 || c->grads_exchanged != 0; }
inline float inv_global_batch(const mpg_train_ctx_t* c) { return 1.f / ((float)c->batch * (float)c->world_size); }
inline float* stats_of(const mpg_train_ctx_t* c, const Layout& l) { return c->grad + l.n_grad; }

// replay_buffer.replay (optimizer.py:340-341; buffer.py:70-91)
int replay_uniform(mpg_train_ctx_t* c, mpg_stream_t s) {
    return mpg_replay_sample_uniform(c->ring_size, c->batch, c->replay_seed, c->replay_times, c->cfg.obs_dim, c->cfg.act_dim, c->ring_obs,
                                     c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done, c->idx, c->b_obs, c->b_act, c->b_rew, c->b_obs2,
                                     c->b_done, s);
}

// sample_iters < 0 asks for |sample_iters| iterations with every chain KEPT (include/mpg_hip.h): the A/B switch of the measurements
// behind the one-launch forms and of the tests that compare the two bit for bit
inline int sample_iters_of(const mpg_train_ctx_t* c) { return c->sample_iters < 0 ? -c->sample_iters : c->sample_iters; }
inline bool one_launch_wanted(const mpg_train_ctx_t* c) { return c->sample_iters > 0; }

// ================================================ the versions' gradients ================================================

// MPGLearner.rule_based_weights, mpg_learner.py:384-399, in float32 like the TF graph
void rule_based_weights(int ite, int total_ite, float eta, const int* select, int ns, float* w) {
    float lam = (1.f - eta) + (2.f * eta / (float)total_ite) * (float)ite;
    lam = std::min(std::max(lam, 0.f), 1.5f);
    int mx = 0;
    for (int k = 0; k < ns; ++k) mx = std::max(mx, select[k]);
    float inv[4], m = -INFINITY;
    for (int k = 0; k < ns; ++k) {
        const float bias = lam < 1.f ? powf(lam, (float)select[k]) : powf(2.f - lam, (float)(mx - select[k]));
        inv[k] = 1.f / (bias + 1e-8f);
        m = std::max(m, inv[k]);
    }
    float sum = 0.f;
    for (int k = 0; k < ns; ++k) { w[k] = expf(inv[k] - m); sum += w[k]; }
    for (int k = 0; k < ns; ++k) w[k] /= sum;
}

// ---- MPGLearner.sample + compute_n_step_target, mpg_learner.py:109-124,146-169 (MPG-v1: networks [Q1 | policy]) ----
int mpg_v1_target(mpg_train_ctx_t* c, const Layout& l, mpg_stream_t s) {
    const int od = c->cfg.obs_dim, ad = c->cfg.act_dim, kind = c->cfg.env_kind;
    const float *policy = c->params + l.off[1], *policy_t = c->targets + l.off[1], *q1t = c->targets;
    TRY(replay_uniform(c, s));
    MPG_REQUIRE(c->l_env_state && c->l_obs && c->l_act && c->l_rewards && c->l_done, "mpg_step_begin: MPG-v1 needs the learner env buffers");
    // The n real-env steps as one launch (bit-identical to the chain below: rewards, last observations, status word) where an entry
    // point serves the configuration; the learner's env state, action and done buffers are not written then.  The pendulum's takes the
    // horizons it serves by the rule of the worker's one-launch samples (tools/bench_env_rollout_pendulum.py).
    const bool ranged_tanh = c->cfg.policy_out_act == MPG_ACT_TANH && c->cfg.action_range > 0.f;
    const bool pendulum = kind == MPG_ENV_INVERTED_PENDULUM;
    if (kind == MPG_ENV_PATH_TRACKING && ad == 2 && c->n < 32 && !ranged_tanh) {
        TRY(mpg_env_rollout(&c->cfg, policy, c->batch, c->n, c->b_obs, c->b_act, c->l_rewards, c->l_obs, s));
    } else if (pendulum && od == 4 && ad == 1 && c->n <= 1024 && !ranged_tanh && one_launch_wanted(c)) {
        TRY(mpg_env_rollout_pendulum(&c->cfg, policy, c->batch, c->n, c->b_obs, c->b_act, c->l_rewards, c->l_obs, s));
    } else {
        TRY(mpg_env_reset_from_obs(kind, c->batch, od, c->l_env_state, c->b_obs, s));
        for (int t = 0; t < c->n; ++t) {
            const float* act = c->b_act;
            if (t > 0) {
                TRY(mpg_policy_action(&c->cfg, policy, c->batch, c->l_obs, 0.f, 0, 0, c->l_act, s));
                act = c->l_act;
            }
            TRY(mpg_env_step(kind, c->batch, od, c->l_env_state, act, c->l_obs, c->l_rewards + (size_t)t * c->batch, c->l_done,
                             c->l_done_intended, s));
        }
    }
    // the pendulum's bootstrap value is clipped (mpg_learner.py:163-164), whichever way the rollout was taken
    if (pendulum)
        return mpg_nstep_targets_clipped(&c->cfg, policy_t, q1t, c->batch, c->n, c->l_rewards, c->l_obs,
                                         MPG_PENDULUM_NSTEP_Q_LO, MPG_PENDULUM_NSTEP_Q_HI, c->b_targets, c->ws0, c->ws0_bytes, s);
    return mpg_nstep_targets(&c->cfg, policy_t, q1t, c->batch, c->n, c->l_rewards, c->l_obs, c->b_targets, c->ws0, c->ws0_bytes, s);
}

// ---- MPGLearner.compute_gradient (mpg_learner.py:401-431), un-clipped partials scaled by 1/B_global.  y_in null: the clipped double-Q
//      target is computed in the first launch; draw non-null: so is the minibatch draw ----
int mpg_gradients(mpg_train_ctx_t* c, const Layout& l, int iteration, const float* y_in, const mpg_replay_draw_t* draw, mpg_stream_t s) {
    float w[4];
    rule_based_weights(iteration, c->total_ite, c->eta, c->select, c->n_select, w);
    // scheduling option (include/mpg_hip.h, mpg_grad_opts_t): with an exchange and the caller's event, the critics' gradient is finished
    // ahead of the reverse sweep.  cfg.grad_opts points at the context for the length of this call only.
    c->grad_opts.critics_ready_event = exchanged(c) ? c->critics_ready_event : nullptr;
    c->cfg.grad_opts = &c->grad_opts;
    const int rc = mpg_mpg_gradients(&c->cfg, l.n_nets - 1, c->params, c->targets, c->batch, c->b_obs, c->b_act, c->b_rew, c->b_obs2, y_in,
                                     c->M, c->n, c->select, c->n_select, w, nullptr, c->learner_seed, c->learner_counter,
                                     inv_global_batch(c), c->grad, stats_of(c, l), c->b_targets, exchanged(c) ? nullptr : c->clip_scratch,
                                     draw, c->ws1, c->ws1_bytes, s);
    c->cfg.grad_opts = nullptr;
    return rc;
}

int mpg_v1_gradients(mpg_train_ctx_t* c, const Layout& l, const Step& st, mpg_stream_t s) {
    if (st.fresh) TRY(mpg_v1_target(c, l, s));
    c->learner_counter++;
    return mpg_gradients(c, l, st.iteration, c->b_targets, nullptr, s);
}

// MPG-v2 (networks [Q1 | Q2 | policy]): the minibatch draw and the clipped double-Q target both ride in the first launch of
// mpg_mpg_gradients; a reused batch keeps the targets it was given then (mpg_learner.py:402-403)
int mpg_v2_gradients(mpg_train_ctx_t* c, const Layout& l, const Step& st, mpg_stream_t s) {
    mpg_replay_draw_t draw = {};
    draw.n_storage = c->ring_size; draw.seed = c->replay_seed; draw.ctr = c->replay_times;
    draw.ring_obs = c->ring_obs; draw.ring_act = c->ring_act; draw.ring_rew = c->ring_rew; draw.ring_obs2 = c->ring_obs2;
    draw.ring_done = c->ring_done; draw.idx_out = c->idx; draw.done_out = c->b_done;
    draw.capacity = c->ring_capacity;
    if (st.predrawn_at >= 0) { draw.pre_gathered = 1; draw.fresh_start = st.predrawn_at; draw.fresh_count = c->num_agent; }
    c->learner_counter++;
    return st.fresh ? mpg_gradients(c, l, st.iteration, nullptr, &draw, s) : mpg_gradients(c, l, st.iteration, c->b_targets, nullptr, s);
}

// ---- NADPLearner.compute_gradient, learners/nadp.py:209-241 (networks [Q1 | policy]) ----
int nadp_gradients(mpg_train_ctx_t* c, const Layout& l, const Step&, mpg_stream_t s) {
    const float *q1 = c->params, *policy = c->params + l.off[1], *q1t = c->targets;
    const float inv_b = inv_global_batch(c);
    float* stats = stats_of(c, l);
    TRY(replay_uniform(c, s));
    c->learner_counter++;
    // n-step model-rollout target from the stored (s, a) (nadp.py:87-126), critic loss (:173-184), policy loss -R_n with the
    // parameter gradient through all n + 1 evaluations (:128-194); noise counters as NADPLearner does (2 k, 2 k + 1)
    TRY(mpg_rollout_q_target(&c->cfg, policy, q1t, c->batch, c->n, c->b_obs, c->b_act, nullptr, c->learner_seed, 2 * c->learner_counter,
                             c->b_targets, c->ws0, c->ws0_bytes, s));
    TRY(mpg_q_loss_grad(&c->cfg, q1, c->batch, c->b_obs, c->b_act, c->b_targets, inv_b, stats, c->grad + l.off[0], nullptr, c->ws0,
                        c->ws0_bytes, s));
    const int sel[2] = {0, c->n};
    const float w[2] = {0.f, 1.f};
    return mpg_rollout_pg(&c->cfg, policy, q1, c->batch, 1, c->n, sel, 2, w, c->b_obs, nullptr, c->learner_seed, 2 * c->learner_counter + 1,
                          inv_b, 1, stats + 2, stats + 4, c->grad + l.off[1], c->ws1, c->ws1_bytes, s);
}

// ---- TD3Learner.compute_gradient, learners/td3.py:150-188 (networks [Q1 | Q2 | policy]) + the priority update of
//      optimizer.py:351-353 ----
int td3_gradients(mpg_train_ctx_t* c, const Layout& l, const Step&, mpg_stream_t s) {
    const int od = c->cfg.obs_dim, ad = c->cfg.act_dim, B = c->batch;
    const float *q1 = c->params, *q2 = c->params + l.off[1], *policy = c->params + l.off[2];
    const float *q1t = c->targets, *q2t = c->targets + l.off[1], *policy_t = c->targets + l.off[2];
    const float inv_b = inv_global_batch(c);
    float* stats = stats_of(c, l);
    float* eps = c->scratch;                          // [B][ad] smoothing noise
    float* y1 = eps + (size_t)B * ad;                 // [B] the priorities' plain Q1 target
    float* td = y1 + B;                               // [B] Q1(s, a) - y
    float* perr = td + B;                             // [B] y1 - Q1(s, a)
    if (c->prioritized)
        TRY(mpg_per_sample_gather(c->per_sum, c->per_min, c->per_capacity, c->ring_size, B, nullptr, c->replay_seed, c->replay_times,
                                  c->per_beta, c->idx, c->b_weights, od, ad, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2,
                                  c->ring_done, c->b_obs, c->b_act, c->b_rew, c->b_obs2, c->b_done, s));
    else
        TRY(replay_uniform(c, s));
    c->learner_counter++;
    TRY(mpg_normal_fill(B * ad, c->learner_seed, c->learner_counter, eps, s));
    TRY(mpg_td3_targets(&c->cfg, policy_t, q1t, q2t, B, c->b_rew, c->b_obs2, eps, c->smooth_sigma, c->smooth_clip, c->b_targets, y1,
                        c->ws0, c->ws0_bytes, s));
    TRY(mpg_q_loss_grad(&c->cfg, q1, B, c->b_obs, c->b_act, c->b_targets, inv_b, stats, c->grad + l.off[0], td, c->ws0, c->ws0_bytes, s));
    TRY(mpg_q_loss_grad(&c->cfg, q2, B, c->b_obs, c->b_act, c->b_targets, inv_b, stats + 1, c->grad + l.off[1], nullptr, c->ws0,
                        c->ws0_bytes, s));
    if (c->prioritized) {
        TRY(mpg_td3_priority_errors(B, y1, c->b_targets, td, perr, s));
        TRY(mpg_per_update(c->per_sum, c->per_min, c->per_stamp, c->per_capacity, B, c->idx, perr, c->per_alpha, c->per_eps,
                           c->per_max_priority, s));
    }
    return mpg_td3_policy_grad(&c->cfg, policy, q1, q2, B, c->b_obs, inv_b, stats + 2, stats + 3, c->grad + l.off[2], c->ws1, c->ws1_bytes, s);
}

// ---- NDPGLearner.compute_gradient, learners/ndpg.py:202-237 (networks [Q1 | policy]); the minibatch and its n-step real-env target
//      (:57-72,127-151) on a fresh call only ----
int ndpg_gradients(mpg_train_ctx_t* c, const Layout& l, const Step& st, mpg_stream_t s) {
    const float *q1 = c->params, *policy = c->params + l.off[1];
    const float inv_b = inv_global_batch(c);
    float* stats = stats_of(c, l);
    c->learner_counter++;
    if (st.fresh) {
        TRY(replay_uniform(c, s));
        TRY(mpg_env_rollout(&c->cfg, policy, c->batch, c->n, c->b_obs, c->b_act, c->l_rewards, c->l_obs, s));
        TRY(mpg_nstep_targets(&c->cfg, c->targets + l.off[1], c->targets, c->batch, c->n, c->l_rewards, c->l_obs, c->b_targets, c->ws0,
                              c->ws0_bytes, s));
    }
    TRY(mpg_q_loss_grad(&c->cfg, q1, c->batch, c->b_obs, c->b_act, c->b_targets, inv_b, stats, c->grad + l.off[0], nullptr, c->ws0,
                        c->ws0_bytes, s));
    return mpg_dpg_policy_grad(&c->cfg, policy, q1, c->batch, c->b_obs, inv_b, stats + 2, stats + 3, c->grad + l.off[1], c->ws1,
                               c->ws1_bytes, s);
}

// ---- SACLearner.compute_gradient, learners/sac.py:169-219 (networks [Q1 | Q2 | policy]); the minibatch and its soft target
//      (:67-80) on a fresh call only.  Draws: counters 2 (k + 1) for the target of call k, 2 k + 1 for the policy loss after
//      the counter's increment, as SACLearner._draw.
//      st.at non-null: the learned temperature - alpha is read on the device (at->state), the _auto entry points run, the third draw
//      (stream learner_seed + 2, the counter after its increment) goes into the second half of the scratch block, the temperature's
//      gradient into grad[n_grad] and the statistics one float further on: [grads | alpha grad | stats] ----
int sac_gradients(mpg_train_ctx_t* c, const Layout& l, const Step& st, mpg_stream_t s) {
    const int ad = c->cfg.act_dim, B = c->batch;
    const float *q1 = c->params, *q2 = c->params + l.off[1], *policy = c->params + l.off[2];
    const float *q1t = c->targets, *q2t = c->targets + l.off[1];
    const mpg_sac_alpha_t* at = st.at;
    const float inv_b = inv_global_batch(c);
    float* stats = stats_of(c, l) + (at ? 1 : 0);
    float* eps = c->scratch;                          // [B][ad]
    if (st.fresh) {
        TRY(replay_uniform(c, s));
        TRY(mpg_normal_fill(B * ad, c->learner_seed, 2 * (c->learner_counter + 1), eps, s));
        if (at)
            TRY(mpg_sac_targets_auto(&c->cfg, policy, q1t, q2t, B, c->b_rew, c->b_obs2, eps, at->state, c->b_targets, c->ws0, c->ws0_bytes, s));
        else
            TRY(mpg_sac_targets(&c->cfg, policy, q1t, q2t, B, c->b_rew, c->b_obs2, eps, st.alpha, c->b_targets, c->ws0, c->ws0_bytes, s));
    }
    c->learner_counter++;
    TRY(mpg_q_loss_grad(&c->cfg, q1, B, c->b_obs, c->b_act, c->b_targets, inv_b, stats, c->grad + l.off[0], nullptr, c->ws0, c->ws0_bytes, s));
    TRY(mpg_q_loss_grad(&c->cfg, q2, B, c->b_obs, c->b_act, c->b_targets, inv_b, stats + 1, c->grad + l.off[1], nullptr, c->ws0,
                        c->ws0_bytes, s));
    TRY(mpg_normal_fill(B * ad, c->learner_seed, 2 * c->learner_counter + 1, eps, s));
    if (at) {
        float* eps_alpha = eps + (size_t)B * ad;
        TRY(mpg_normal_fill(B * ad, c->learner_seed + 2, c->learner_counter, eps_alpha, s));
        return mpg_sac_policy_grad_auto(&c->cfg, policy, q1, q2, B, c->b_obs, eps, at->state, eps_alpha, at->target_entropy, inv_b, stats + 2,
                                        stats + 3, stats + 4, c->grad + l.n_grad, c->grad + l.off[2], c->ws1, c->ws1_bytes, s);
    }
    return mpg_sac_policy_grad(&c->cfg, policy, q1, q2, B, c->b_obs, eps, st.alpha, inv_b, stats + 2, stats + 3, stats + 4,
                               c->grad + l.off[2], c->ws1, c->ws1_bytes, s);
}

// ---- AMPCLearner.compute_gradient, learners/ampc.py:105-122 (networks [policy]): the statistics are the two return sums; the noise
//      counter is the one AMPCLearner uses after _begin has counted the call ----
int ampc_gradients(mpg_train_ctx_t* c, const Layout& l, const Step&, mpg_stream_t s) {
    float* stats = stats_of(c, l);
    TRY(replay_uniform(c, s));
    c->learner_counter++;
    return mpg_ampc_pg(&c->cfg, c->params, c->batch, c->M, c->n, c->b_obs, nullptr, c->learner_seed, 2 * c->learner_counter + 1,
                       inv_global_batch(c), stats, stats + 1, c->grad, c->ws1, c->ws1_bytes, s);
}

// ================================================ the table of versions ================================================

// what mpg_ampc_pg would refuse of (cfg, batch, M, n), said under the caller's name BEFORE the sample runs
int ampc_shape_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c->batch > 0, "%s: learner_version 8 (AMPC): no rows (batch %d)", entry, c->batch);
    MPG_REQUIRE(c->M > 0, "%s: learner_version 8 (AMPC): M must be positive (got %d)", entry, c->M);
    MPG_REQUIRE(c->n > 0 && c->n < 32, "%s: learner_version 8 (AMPC): horizon out of range: 0 < n < 32 (got %d)", entry, c->n);
    const long R = (long)c->batch * c->M;
    MPG_REQUIRE(R % 16 == 0, "%s: learner_version 8 (AMPC): every step is differentiated through the policy: needs batch*M %% 16 == 0 (got %ld)",
                entry, R);
    MPG_REQUIRE(mpg_ampc_pg_workspace_bytes(&c->cfg, c->batch, c->M, c->n) != 0,
                "%s: learner_version 8 (AMPC): unsupported cfg (obs/act dims, env_kind) for mpg_ampc_pg", entry);
    return MPG_OK;
}

// ws0: targets / critic loss; ws1: the policy gradient
inline size_t critic_ws0(const mpg_train_ctx_t* c) {
    return std::max(mpg_q_targets_workspace_bytes(&c->cfg, c->batch), mpg_q_loss_grad_workspace_bytes(&c->cfg, c->batch));
}
void mpg_workspace(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    *ws0 = critic_ws0(c);
    *ws1 = mpg_mpg_gradients_workspace_bytes(&c->cfg, c->batch, c->M, c->n, c->n_select, traits(c->learner_version)->n_critics);
}
void nadp_workspace(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    *ws0 = critic_ws0(c);
    *ws0 = std::max(*ws0, mpg_rollout_q_target_workspace_bytes(&c->cfg, c->batch));
    *ws1 = mpg_rollout_pg_workspace_bytes(&c->cfg, c->batch, 1, c->n, 2, 1);
}
void td3_workspace(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    *ws0 = critic_ws0(c);
    *ws1 = mpg_td3_policy_grad_workspace_bytes(&c->cfg, c->batch);
}
void ndpg_workspace(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    *ws0 = critic_ws0(c);
    *ws1 = mpg_dpg_policy_grad_workspace_bytes(&c->cfg, c->batch);
}
void sac_workspace(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    *ws0 = std::max(mpg_sac_targets_workspace_bytes(&c->cfg, c->batch), mpg_q_loss_grad_workspace_bytes(&c->cfg, c->batch));
    *ws1 = mpg_sac_policy_grad_workspace_bytes(&c->cfg, c->batch);
}
void ampc_workspace(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {      // no target and no critic: the rollout gradient alone
    *ws0 = 0;
    *ws1 = mpg_ampc_pg_workspace_bytes(&c->cfg, c->batch, c->M, c->n);
}

// (n_q + 2 n_select statistics in 8 slots: three horizons at most with one critic or two)
bool mpg_complete(const mpg_train_ctx_t* c) { return c->n > 0 && c->M > 0 && c->n_select > 0 && c->n_select <= 3; }
bool nadp_complete(const mpg_train_ctx_t* c) { return c->n > 0; }
// the scratch block, and the trees when the replay is prioritized
bool td3_complete(const mpg_train_ctx_t* c) {
    return c->scratch && (!c->prioritized || (c->per_sum && c->per_min && c->per_stamp && c->per_capacity >= c->ring_capacity &&
                                              c->per_max_priority && c->b_weights));
}
bool ndpg_complete(const mpg_train_ctx_t* c) { return c->n > 0 && c->l_obs && c->l_rewards; }       // no state block, no l_act / l_done*
bool sac_complete(const mpg_train_ctx_t* c) { return c->scratch != nullptr; }                       // the draws' block
// (mpg_step_begin has said what is wrong in words of its own - ampc_refusal - before it asks here)
bool ampc_complete(const mpg_train_ctx_t* c) { return c->n > 0 && c->M > 0 && !c->prioritized; }

constexpr Traits VERSIONS[AMPC + 1] = {
    //        critics target reuse  PER    stoch. predraw partials
    {},
    /* MPG_V1 */ {1, true,  true,  false, false, false, true,  mpg_complete,  mpg_workspace,  mpg_v1_gradients},
    /* MPG_V2 */ {2, true,  true,  false, false, true,  true,  mpg_complete,  mpg_workspace,  mpg_v2_gradients},
    /* NADP   */ {1, true,  false, false, false, false, false, nadp_complete, nadp_workspace, nadp_gradients},
    /* TD3    */ {2, true,  false, true,  false, false, false, td3_complete,  td3_workspace,  td3_gradients},
    /* NDPG   */ {1, true,  true,  false, false, false, false, ndpg_complete, ndpg_workspace, ndpg_gradients},
    /* 6 is not assigned */ {},
    /* SAC    */ {2, true,  true,  false, true,  false, false, sac_complete,  sac_workspace,  sac_gradients},
    /* AMPC   */ {0, false, false, false, false, false, false, ampc_complete, ampc_workspace, ampc_gradients},
};
const Traits* traits(int version) { return version >= MPG_V1 && version <= AMPC && VERSIONS[version].gradients ? &VERSIONS[version] : nullptr; }

Layout layout(const mpg_train_ctx_t* c, const Traits& t) {
    Layout l;
    l.q_size = net_size(c->cfg.obs_dim + c->cfg.act_dim, 1);
    l.p_size = net_size(c->cfg.obs_dim, 2 * c->cfg.act_dim);
    l.n_nets = t.n_critics + 1;
    int o = 0;
    for (int k = 0; k < l.n_nets; ++k) {
        l.sizes[k] = k == l.n_nets - 1 ? l.p_size : l.q_size;
        l.off[k] = o;
        o += l.sizes[k];
    }
    l.n_grad = o;
    return l;
}

bool ctx_ok(const mpg_train_ctx_t* c) {
    const Traits* t = c ? traits(c->learner_version) : nullptr;
    return t && c->num_agent > 0 && c->batch > 0 && c->world_size > 0 && c->sampling_interval > 0 && c->ring_capacity > 0 &&
           c->num_batch_reuse > 0 && (t->batch_reuse || c->num_batch_reuse == 1) && c->params && c->targets && c->grad &&
           (c->ws0 || !t->n_critics) && c->ws1 && t->complete(c);
}

// ================================================ refusals ================================================

// the driver's first act is the worker's sample on the REAL env, which this model does not have
int real_env_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c->cfg.env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM,
                "%s: the real InvertedDoublePendulum-v2 env is MuJoCo and is not provided, so the native step driver (which "
                "samples it) does not serve this model; use the rollout entry points (NADPLearner) on caller-supplied batches", entry);
    return MPG_OK;
}

// everything mpg_step_begin refuses of an AMPC context, each with its own text, before anything is enqueued or any counter moves
int ampc_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c->num_agent > 0 && c->batch > 0 && c->world_size > 0 && c->sampling_interval > 0 && c->ring_capacity > 0,
                "%s: incomplete context (learner_version 8: num_agent %d, batch %d, world_size %d, sampling_interval %d, ring_capacity %d "
                "must all be positive)", entry, c->num_agent, c->batch, c->world_size, c->sampling_interval, c->ring_capacity);
    TRY(real_env_refusal(entry, c));
    MPG_REQUIRE(c->num_batch_reuse == 1, "%s: learner_version 8 (AMPC) draws a fresh batch on every call: num_batch_reuse must be 1 (got %d)",
                entry, c->num_batch_reuse);
    MPG_REQUIRE(!c->prioritized, "%s: learner_version 8 (AMPC): a prioritized replay buffer is not served (prioritized = %d)", entry,
                c->prioritized);
    TRY(ampc_shape_refusal(entry, c));
    MPG_REQUIRE(c->num_agent <= c->ring_capacity, "%s: ring smaller than one sample", entry);
    const struct { const char* name; const void* p; } need[] = {
        {"params", c->params}, {"targets", c->targets}, {"grad", c->grad}, {"ws1", c->ws1},
        {"env_state", c->env_state}, {"w_obs", c->w_obs}, {"w_act", c->w_act}, {"w_done", c->w_done},
        {"ring_obs", c->ring_obs}, {"ring_act", c->ring_act}, {"ring_rew", c->ring_rew}, {"ring_obs2", c->ring_obs2}, {"ring_done", c->ring_done},
        {"idx", c->idx}, {"b_obs", c->b_obs}, {"b_act", c->b_act}, {"b_rew", c->b_rew}, {"b_obs2", c->b_obs2}, {"b_done", c->b_done}};
    for (const auto& q : need) MPG_REQUIRE(q.p, "%s: learner_version 8 (AMPC): null pointer: %s", entry, q.name);
    const size_t ws1 = mpg_ampc_pg_workspace_bytes(&c->cfg, c->batch, c->M, c->n);
    if (c->ws1_bytes < ws1) {
        mpg_set_error("%s: learner_version 8 (AMPC): ws1 too small for mpg_ampc_pg (%zu < %zu)", entry, c->ws1_bytes, ws1);
        return MPG_EWORKSPACE;
    }
    return MPG_OK;
}

// what mpg_sac_step_begin and mpg_sac_auto_step_begin refuse alike, under the caller's name
int sac_begin_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c, "%s: null context", entry);
    MPG_REQUIRE(c->learner_version == SAC, "%s: learner_version 7 (SAC) only (got %d)", entry, c->learner_version);
    MPG_REQUIRE(ctx_ok(c), "%s: incomplete context", entry);
    MPG_REQUIRE(!c->prioritized, "%s: a prioritized replay buffer is not served (prioritized = %d)", entry, c->prioritized);
    MPG_REQUIRE(c->explore_sigma == 0.f, "%s: explore_sigma on top of the stochastic policy is not served (got %g)", entry,
                (double)c->explore_sigma);
    return MPG_OK;
}

// ================================================ the worker's sample ================================================
// worker.sample + replay_buffer.add_batch (optimizer.py:332-337, worker.py:68-79,91-119): sample_iters iterations of policy (+ noise, or
// the Gaussian head's draw) -> env.step -> ring slot (next + i) % capacity -> env.reset of the done agents.

// The iteration as ONE launch, mpg_worker_step: path-tracking env, six-entry observations.  mpg_worker_step serves obs_dim 7 .. 16
// too; the driver does not take it there: its step time against the two launches at K = 3 / 10 has NOT been measured
inline bool worker_step_fused(const mpg_train_ctx_t* c) {
    return c->cfg.env_kind == MPG_ENV_PATH_TRACKING && c->cfg.obs_dim == 6 && c->cfg.act_dim == 2;
}
inline bool pendulum_worker(const mpg_train_ctx_t* c) {
    return c->cfg.env_kind == MPG_ENV_INVERTED_PENDULUM && c->cfg.obs_dim == 4 && c->cfg.act_dim == 1;
}

// How many leading iterations of a sample go as ONE launch (each bit-identical to its chain): all of them, but the one that pre-draws,
// when there are at least two (and at most the 1024 a launch takes) and the ring holds them all (iters * n <= capacity is what the
// launch asks: no slot written twice).  The entry points: mpg_worker_sample_rollout at every width (tools/bench_worker_rollout.py
// --stochastic), mpg_worker_rollout where mpg_worker_step is taken (f9), mpg_worker_rollout_pendulum (--env pendulum;
// f10) - per width, the launch's median at or below the chain's at both measured sizes is the rule for taking it.
int one_launch_iters(const mpg_train_ctx_t* c, const Traits& t, bool last_predraws) {
    const int k = sample_iters_of(c) - (last_predraws ? 1 : 0);
    const bool served = t.stochastic || worker_step_fused(c) || pendulum_worker(c);
    return one_launch_wanted(c) && served && k >= 2 && k <= 1024 && (long)k * c->num_agent <= c->ring_capacity ? k : 0;
}

// an iteration's transitions are in the ring: they enter the trees at the max priority (buffer.py:127-136; mpg_per_add reads no ring
// row and the worker's launch reads no tree), and the ring position moves on
int iteration_added(mpg_train_ctx_t* c, const Traits& t, mpg_stream_t s) {
    if (t.prioritized && c->prioritized)
        TRY(mpg_per_add(c->per_sum, c->per_min, c->per_stamp, c->per_capacity, c->ring_capacity, c->ring_next, c->num_agent, c->per_alpha,
                        c->per_max_priority, reinterpret_cast<int*>(c->scratch), s));
    c->ring_next = (c->ring_next + c->num_agent) % c->ring_capacity;
    c->ring_size = std::min(c->ring_size + c->num_agent, c->ring_capacity);
    return MPG_OK;
}

// predrawn_at non-null: the caller draws its minibatch right after the add.  The last launch then gathers it in spare workgroups (the
// random ring reads overlap the env's sub-steps) except the rows drawn from the slots that launch is writing - where mpg_worker_step is
// taken - and *predrawn_at becomes the first of those slots.
int sample(const char* entry, mpg_train_ctx_t* c, const Traits& t, const float* policy, int* predrawn_at, mpg_stream_t s) {
    const int n = c->num_agent, iters = sample_iters_of(c);
    // (a deterministic worker asked for no iteration stores nothing and passes; the stochastic one's ring is looked at regardless)
    MPG_REQUIRE(n <= c->ring_capacity || (iters == 0 && !t.stochastic), "%s: ring smaller than one sample", entry);
    const bool predraws = predrawn_at && worker_step_fused(c);
    int it = one_launch_iters(c, t, predraws);
    if (it) {
        if (t.stochastic) {
            TRY(mpg_worker_sample_rollout(&c->cfg, policy, n, it, c->env_state, c->w_obs, c->worker_seed, c->noise_ctr, c->w_act,
                                          c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                          c->env_seed, c->env_ctr, c->w_done, s));
        } else {
            const auto rollout = pendulum_worker(c) ? mpg_worker_rollout_pendulum : mpg_worker_rollout;      // (one signature)
            TRY(rollout(&c->cfg, policy, n, it, c->env_state, c->w_obs, c->explore_sigma, c->worker_seed, c->noise_ctr, c->w_act,
                        c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done, c->env_seed,
                        c->env_ctr, c->w_done, s));
        }
        c->noise_ctr += it;
        c->env_ctr += it;
        for (int k = 0; k < it; ++k) TRY(iteration_added(c, t, s));       // in iteration order, as the chain does
    }
    for (; it < iters; ++it) {
        if (t.stochastic) {        // one launch at every width; the log-densities have no consumer: worker.py:96 drops them
            TRY(mpg_worker_sample_step(&c->cfg, policy, n, c->env_state, c->w_obs, c->worker_seed, c->noise_ctr++, c->w_act, nullptr,
                                       c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                       c->env_seed, c->env_ctr++, c->w_done, s));
        } else if (worker_step_fused(c)) {
            mpg_replay_draw_t pd = {};
            const bool predraw = predraws && it == iters - 1;
            if (predraw) {
                pd.n_storage = std::min(c->ring_size + n, c->ring_capacity);
                pd.seed = c->replay_seed; pd.ctr = c->replay_times + 1;
                pd.idx_out = c->idx; pd.done_out = c->b_done;
                *predrawn_at = c->ring_next;
            }
            TRY(mpg_worker_step(&c->cfg, policy, n, c->env_state, c->w_obs, c->explore_sigma, c->worker_seed, c->noise_ctr++, c->w_act,
                                c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                c->env_seed, c->env_ctr++, c->w_done, predraw ? &pd : nullptr, c->batch, c->b_obs, c->b_act, c->b_rew,
                                c->b_obs2, s));
        } else {
            TRY(mpg_policy_action(&c->cfg, policy, n, c->w_obs, c->explore_sigma, c->worker_seed, c->noise_ctr++, c->w_act, s));
            mpg_prof_begin(c->cfg.prof, 2, mpg_stream(s));
            TRY(mpg_env_step_store_reset(c->cfg.env_kind, n, c->cfg.obs_dim, c->env_state, c->w_act, c->ring_capacity, c->ring_next,
                                         c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done, c->env_seed, c->env_ctr++,
                                         c->w_obs, c->w_done, s));
            mpg_prof_end(c->cfg.prof, 2, mpg_stream(s));
        }
        TRY(iteration_added(c, t, s));
    }
    return MPG_OK;
}

// ================================================ the begin skeleton ================================================
// optimizer.py:330-353: sample and add on the interval, replay, the version's gradients.  The caller has made its refusals.
int begin(const char* entry, mpg_train_ctx_t* c, int iteration, float alpha, const mpg_sac_alpha_t* at, mpg_stream_t s) {
    const Traits& t = *traits(c->learner_version);
    const Layout l = layout(c, t);
    Step st = {iteration, c->learner_counter % c->num_batch_reuse == 0, -1, alpha, at};
    if (iteration % c->sampling_interval == 0)
        TRY(sample(entry, c, t, c->params + l.off[l.n_nets - 1], t.predraw && st.fresh ? &st.predrawn_at : nullptr, s));
    MPG_REQUIRE(c->ring_size > 0, "%s: empty replay ring", entry);
    c->replay_times++;
    return t.gradients(c, l, st, s);
}

// what mpg_step_begin refuses, under the caller's name (mpg_step_begin_lagged refuses the same)
int step_begin_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(!c || c->learner_version != SAC,
                "%s: learner_version 7 (SAC) takes its temperature as an argument: call mpg_sac_step_begin", entry);
    if (c && c->learner_version == AMPC) TRY(ampc_refusal(entry, c));      // each refusal in its own words; ctx_ok then holds
    MPG_REQUIRE(ctx_ok(c), "%s: incomplete context", entry);
    return real_env_refusal(entry, c);                              // refused before anything is enqueued
}
int sac_fixed_refusal(const char* entry, const mpg_train_ctx_t* c, float alpha) {
    TRY(sac_begin_refusal(entry, c));
    MPG_REQUIRE(alpha >= 0.f && alpha <= 3.4028234664e38f, "%s: alpha must be finite and not negative (got %g)", entry, (double)alpha);
    return real_env_refusal(entry, c);
}
int sac_auto_refusal(const char* entry, const mpg_train_ctx_t* c, const mpg_sac_alpha_t* a) {
    TRY(sac_begin_refusal(entry, c));
    MPG_REQUIRE(a, "%s: null temperature struct", entry);
    MPG_REQUIRE(a->state, "%s: null temperature state", entry);
    MPG_REQUIRE(std::isfinite(a->target_entropy), "%s: target_entropy must be finite (got %g)", entry, (double)a->target_entropy);
    return real_env_refusal(entry, c);
}

// ================================================ the lagged sample ================================================
// sample_lag = L (include/mpg_hip.h, mpg_lagged_sample_t): the sample that starts at iteration k reads the policy as it stands at the
// start of k and its rows enter the ring at the start of k + L.  In between they sit in the object's staging rows, written by the
// sample's launches on the side stream; the worker's counters move at k, the ring's at k + L.

inline bool two_streams(const mpg_lagged_sample_t* g, mpg_stream_t s) { return g->side && g->side != s; }

// what the lagged form refuses beyond its version's begin, before anything is enqueued or counted (the context has passed that begin's
// refusals: it is complete)
int lagged_refusal(const char* entry, const mpg_train_ctx_t* c, const mpg_lagged_sample_t* g, mpg_stream_t s) {
    MPG_REQUIRE(g->lag >= 1 && g->lag <= c->sampling_interval, "%s: lag out of range: 1 <= lag <= sampling_interval = %d (got %d)", entry,
                c->sampling_interval, g->lag);
    MPG_REQUIRE(g->s_obs && g->s_act && g->s_rew && g->s_obs2 && g->s_done,
                "%s: missing staging rows (s_obs, s_act, s_rew, s_obs2, s_done: |sample_iters| * num_agent rows each)", entry);
    MPG_REQUIRE(g->policy, "%s: missing policy copy (the worker's own net_size(policy) floats)", entry);
    MPG_REQUIRE(!(c->cfg.prof && two_streams(g, s)), "%s: a kernel timer (cfg.prof) records on one stream: not served with a side stream",
                entry);
    MPG_REQUIRE(!two_streams(g, s) || (g->forked && g->done), "%s: a side stream needs both events (forked, done)", entry);
    MPG_REQUIRE(c->world_size == 1, "%s: world_size > 1 is not served with a lagged sample (got %d)", entry, c->world_size);
    MPG_REQUIRE(sample_iters_of(c) > 0, "%s: a lagged sample of no iteration (sample_iters = 0)", entry);
    MPG_REQUIRE((long)sample_iters_of(c) * c->num_agent <= c->ring_capacity, "%s: ring smaller than one sample", entry);
    MPG_REQUIRE(g->pending >= 0 && g->pending <= sample_iters_of(c), "%s: pending count out of range (got %d)", entry, g->pending);
    return MPG_OK;
}

// the staged rows enter the ring (and the trees, iteration by iteration) on the MAIN stream, behind the sample's last launch
int join(const char* entry, mpg_train_ctx_t* c, const Traits& t, mpg_lagged_sample_t* g, mpg_stream_t s) {
    if (two_streams(g, s)) HIP_TRY(entry, hipStreamWaitEvent(mpg_stream(s), static_cast<hipEvent_t>(g->done), 0));
    TRY(mpg_replay_add(c->ring_capacity, c->ring_next, g->pending * c->num_agent, c->cfg.obs_dim, c->cfg.act_dim, g->s_obs, g->s_act,
                       g->s_rew, g->s_obs2, g->s_done, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done, s));
    for (int k = 0; k < g->pending; ++k) TRY(iteration_added(c, t, s));
    g->pending = 0;
    return MPG_OK;
}

// The policy's floats go into the worker's copy on the MAIN stream, ahead of the fork event: the step's own optimizer launch
// (mpg_step_end of this iteration) writes them, and nothing orders it behind a copy made on the side stream.  The sample's launches then
// run on the side stream with the staging rows as their ring (capacity = the rows of one sample, position 0: what
// OffPolicyWorker._one_launch hands them), reading the copy alone (it matches no packed image: the strided loads, bit-identical).
// MPG-v2's pre-gathered draw is not taken: the draw does not follow this add.
int fork(const char* entry, mpg_train_ctx_t* c, const Traits& t, const Layout& l, mpg_lagged_sample_t* g, int iteration, mpg_stream_t s) {
    const bool two = two_streams(g, s);
    const mpg_stream_t side = two ? g->side : s;
    HIP_TRY(entry, hipMemcpyAsync(g->policy, c->params + l.off[l.n_nets - 1], sizeof(float) * (size_t)l.p_size, hipMemcpyDeviceToDevice,
                                  mpg_stream(s)));
    if (two) {
        HIP_TRY(entry, hipEventRecord(static_cast<hipEvent_t>(g->forked), mpg_stream(s)));
        HIP_TRY(entry, hipStreamWaitEvent(mpg_stream(side), static_cast<hipEvent_t>(g->forked), 0));
    }
    mpg_train_ctx_t w = *c;
    w.ring_obs = g->s_obs; w.ring_act = g->s_act; w.ring_rew = g->s_rew; w.ring_obs2 = g->s_obs2; w.ring_done = g->s_done;
    w.ring_capacity = sample_iters_of(c) * c->num_agent;
    w.ring_next = w.ring_size = 0;
    w.prioritized = 0;                      // the trees are the join's
    TRY(sample(entry, &w, t, g->policy, nullptr, side));
    c->noise_ctr = w.noise_ctr;
    c->env_ctr = w.env_ctr;
    if (two) HIP_TRY(entry, hipEventRecord(static_cast<hipEvent_t>(g->done), mpg_stream(side)));
    g->pending = sample_iters_of(c);
    g->due = iteration + g->lag;
    return MPG_OK;
}

// begin with the add moved on: join what is due, fork on the interval, the version's gradients.  The caller has made its refusals.
int begin_lagged(const char* entry, mpg_train_ctx_t* c, mpg_lagged_sample_t* g, int iteration, float alpha, const mpg_sac_alpha_t* at,
                 mpg_stream_t s) {
    TRY(lagged_refusal(entry, c, g, s));
    const Traits& t = *traits(c->learner_version);
    const Layout l = layout(c, t);
    const bool due = g->pending > 0 && iteration >= g->due, forks = iteration % c->sampling_interval == 0;
    MPG_REQUIRE(!(forks && g->pending > 0 && !due), "%s: the sample due at iteration %d is still pending at a sampling iteration (%d)",
                entry, g->due, iteration);
    MPG_REQUIRE(c->ring_size > 0 || due, "%s: empty replay ring", entry);
    const Step st = {iteration, c->learner_counter % c->num_batch_reuse == 0, -1, alpha, at};
    if (due) TRY(join(entry, c, t, g, s));
    if (forks) TRY(fork(entry, c, t, l, g, iteration, s));
    c->replay_times++;
    return t.gradients(c, l, st, s);
}

// the end's own requirements, under the caller's name
bool end_ok(const mpg_train_ctx_t* c) { return ctx_ok(c) && c->norms && c->nonfinite && c->adam_m && c->adam_v && c->clip_scratch; }

}  // namespace

extern "C" int mpg_step_workspace_bytes(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    MPG_REQUIRE(c && ws0 && ws1, "mpg_step_workspace_bytes: null pointer");
    const Traits* t = traits(c->learner_version);
    MPG_REQUIRE(t, "mpg_step_workspace_bytes: unknown learner_version %d", c->learner_version);
    if (c->learner_version == AMPC) TRY(ampc_shape_refusal("mpg_step_workspace_bytes", c));      // in its own words, as mpg_step_begin
    t->workspace(c, ws0, ws1);
    MPG_REQUIRE((*ws0 || !t->n_critics) && *ws1, "mpg_step_workspace_bytes: unsupported configuration");
    return MPG_OK;
}

extern "C" int mpg_step_begin(mpg_train_ctx_t* c, int iteration, mpg_stream_t s) {
    TRY(step_begin_refusal("mpg_step_begin", c));
    return begin("mpg_step_begin", c, iteration, 0.f, nullptr, s);
}

extern "C" int mpg_sac_step_begin(mpg_train_ctx_t* c, float alpha, int iteration, mpg_stream_t s) {
    TRY(sac_fixed_refusal("mpg_sac_step_begin", c, alpha));
    return begin("mpg_sac_step_begin", c, iteration, alpha, nullptr, s);
}

extern "C" int mpg_sac_auto_step_begin(mpg_train_ctx_t* c, const mpg_sac_alpha_t* a, int iteration, mpg_stream_t s) {
    TRY(sac_auto_refusal("mpg_sac_auto_step_begin", c, a));
    return begin("mpg_sac_auto_step_begin", c, iteration, 0.f, a, s);
}

// ---- the same three with a lagged sample (include/mpg_hip.h, mpg_lagged_sample_t) ----
extern "C" int mpg_step_begin_lagged(mpg_train_ctx_t* c, mpg_lagged_sample_t* g, int iteration, mpg_stream_t s) {
    MPG_REQUIRE(g, "mpg_step_begin_lagged: null lagged-sample object");
    TRY(step_begin_refusal("mpg_step_begin_lagged", c));
    return begin_lagged("mpg_step_begin_lagged", c, g, iteration, 0.f, nullptr, s);
}

extern "C" int mpg_sac_step_begin_lagged(mpg_train_ctx_t* c, float alpha, mpg_lagged_sample_t* g, int iteration, mpg_stream_t s) {
    MPG_REQUIRE(g, "mpg_sac_step_begin_lagged: null lagged-sample object");
    TRY(sac_fixed_refusal("mpg_sac_step_begin_lagged", c, alpha));
    return begin_lagged("mpg_sac_step_begin_lagged", c, g, iteration, alpha, nullptr, s);
}

extern "C" int mpg_sac_auto_step_begin_lagged(mpg_train_ctx_t* c, const mpg_sac_alpha_t* a, mpg_lagged_sample_t* g, int iteration,
                                              mpg_stream_t s) {
    MPG_REQUIRE(g, "mpg_sac_auto_step_begin_lagged: null lagged-sample object");
    TRY(sac_auto_refusal("mpg_sac_auto_step_begin_lagged", c, a));
    return begin_lagged("mpg_sac_auto_step_begin_lagged", c, g, iteration, 0.f, a, s);
}

// a pending sample is joined and added now, whatever its due iteration: the end of a run
extern "C" int mpg_lagged_sample_drain(mpg_train_ctx_t* c, mpg_lagged_sample_t* g, mpg_stream_t s) {
    MPG_REQUIRE(g, "mpg_lagged_sample_drain: null lagged-sample object");
    MPG_REQUIRE(ctx_ok(c), "mpg_lagged_sample_drain: incomplete context");
    TRY(lagged_refusal("mpg_lagged_sample_drain", c, g, s));
    return g->pending > 0 ? join("mpg_lagged_sample_drain", c, *traits(c->learner_version), g, s) : MPG_OK;
}

extern "C" int mpg_step_end(mpg_train_ctx_t* c, int iteration, mpg_stream_t s) {
    MPG_REQUIRE(end_ok(c), "mpg_step_end: incomplete context");
    const Traits& t = *traits(c->learner_version);
    const Layout l = layout(c, t);
    // per-network clip_by_global_norm (mpg_learner.py:415-431): on one GPU a gradient launch that leaves the partial sums of squares
    // (mpg_mpg_gradients) has put them into clip_scratch; otherwise, and after an all-reduce, they are taken from the gradient buffer -
    // unless the exchange summed with mpg_sum_slots_sq and has left them already (clip_partials_ready)
    if (exchanged(c) ? !c->clip_partials_ready : !t.clip_partials) TRY(mpg_sq_partials(c->grad, l.sizes, l.n_nets, c->clip_scratch, s));
    // PolicyWithQs.apply_gradients, policy.py:123-156 (without a target there is no delay either: delay_update and tau are not looked at)
    const bool delayed = !t.target || iteration % c->delay_update == 0;
    float lr_t[3];
    int do_adam[3], do_polyak[3];
    for (int k = 0; k < l.n_nets; ++k) {
        const bool is_policy = k == l.n_nets - 1;
        const bool upd = !is_policy || delayed;
        lr_t[k] = adam_step_size(is_policy ? c->policy_lr : c->value_lr, c->opt_steps[k]);
        do_adam[k] = upd ? 1 : 0;
        do_polyak[k] = delayed && t.target ? 1 : 0;
        if (upd) c->opt_steps[k]++;
    }
    mpg_prof_begin(c->cfg.prof, 9, mpg_stream(s));
    const int rc = mpg_clip_adam_polyak(c->params, c->adam_m, c->adam_v, c->targets, c->grad, c->clip_scratch, l.sizes, l.n_nets, c->clip,
                                        lr_t, do_adam, do_polyak, c->tau, c->norms, c->nonfinite, c->cfg.wcache[0], c->cfg.wcache[1], s);
    mpg_prof_end(c->cfg.prof, 9, mpg_stream(s));
    return rc;
}

// mpg_step_end for the learned temperature: the networks' clip + Adam + Polyak as for every version (the segments end where the
// temperature's gradient begins), then the temperature's one launch - its clip and snapshot, and its Adam step together with the
// policy's (policy.py:136-143), with a zero gradient if a network's gradient was not finite (ctx->nonfinite, written by the launch before)
extern "C" int mpg_sac_auto_step_end(mpg_train_ctx_t* c, mpg_sac_alpha_t* a, int iteration, mpg_stream_t s) {
    MPG_REQUIRE(c, "mpg_sac_auto_step_end: null context");
    MPG_REQUIRE(c->learner_version == SAC, "mpg_sac_auto_step_end: learner_version 7 (SAC) only (got %d)", c->learner_version);
    MPG_REQUIRE(a, "mpg_sac_auto_step_end: null temperature struct");
    MPG_REQUIRE(a->state, "mpg_sac_auto_step_end: null temperature state");
    MPG_REQUIRE(end_ok(c), "mpg_sac_auto_step_end: incomplete context");
    MPG_REQUIRE(c->clip > 0.f && a->opt_steps >= 0, "mpg_sac_auto_step_end: clip norm %g / temperature step counter %lld", (double)c->clip,
                a->opt_steps);
    const Layout l = layout(c, *traits(SAC));
    TRY(mpg_step_end(c, iteration, s));
    return mpg_sac_alpha_update(a, c->grad + l.n_grad, c->clip, 1, iteration % c->delay_update == 0 ? 1 : 0, c->nonfinite, l.n_nets, s);
}
