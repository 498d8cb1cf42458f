// Native step driver: SingleProcessOffPolicyOptimizer.step (optimizer.py:330-362) for the MPG learner, built purely
// from the public entry points of this library so that Python is not on the launch path.
#include <algorithm>
#include <cmath>

#include "adam_schedule.h"
#include "mpg_common.h"

namespace {

constexpr int H = MPG_HIDDEN;
inline int net_size(int in_dim, int out_dim) { return in_dim * H + H + H * H + H + H * out_dim + out_dim; }

struct Layout {
    int n_nets, q_size, p_size, n_grad;
    int sizes[3], off[3];   // Q1, (Q2), policy
};

Layout layout(const mpg_train_ctx_t* c) {
    Layout l;
    l.q_size = net_size(c->cfg.obs_dim + c->cfg.act_dim, 1);
    l.p_size = net_size(c->cfg.obs_dim, 2 * c->cfg.act_dim);
    l.n_nets = (c->learner_version == 2 || c->learner_version == 4 || c->learner_version == 7) ? 3 : 2;        // MPG-v2 / TD3 / SAC: double Q
    if (c->learner_version == 8) l.n_nets = 1;                                                                 // AMPC: the policy alone
    int o = 0;
    for (int k = 0; k < l.n_nets; ++k) {
        l.sizes[k] = k == l.n_nets - 1 ? l.p_size : l.q_size;
        l.off[k] = o;
        o += l.sizes[k];
    }
    l.n_grad = o;
    return l;
}

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

// (polynomial_decay, adam_step_size: adam_schedule.h)

#define TRY(call)            \
    do {                     \
        int rc_ = (call);    \
        if (rc_) return rc_; \
    } while (0)

inline bool exchanged(const mpg_train_ctx_t* c) { return c->world_size > 1 || c->grads_exchanged != 0; }

inline bool is_mpg(const mpg_train_ctx_t* c) { return c->learner_version == 1 || c->learner_version == 2; }
inline bool is_ampc(const mpg_train_ctx_t* c) { return c->learner_version == 8; }

bool ctx_ok(const mpg_train_ctx_t* c) {
    if (!c || c->learner_version < 1 || c->learner_version == 6 || c->learner_version > 8) return false;
    // AMPC: no critic and no target, so no ws0; mpg_step_begin has said what is wrong in words of its own (ampc_refusal) before it asks here
    if (is_ampc(c))
        return c->num_agent > 0 && c->batch > 0 && c->world_size > 0 && c->sampling_interval > 0 && c->num_batch_reuse == 1 &&
               c->ring_capacity > 0 && c->params && c->targets && c->grad && c->ws1 && c->n > 0 && c->M > 0 && !c->prioritized;
    const bool common = c->num_agent > 0 && c->batch > 0 && c->world_size > 0 && c->sampling_interval > 0 && c->num_batch_reuse > 0 &&
                        c->ring_capacity > 0 && c->params && c->targets && c->grad && c->ws0 && c->ws1;
    if (!common) return false;
    if (is_mpg(c))
        return c->n > 0 && c->M > 0 && c->n_select > 0 && c->n_select <= 4 && (c->learner_version == 2 ? 2 : 1) + 2 * c->n_select <= 8;
    if (c->learner_version == 3) return c->n > 0 && c->num_batch_reuse == 1;
    if (c->learner_version == 5) return c->n > 0 && c->l_obs && c->l_rewards;       // no state block, no l_act / l_done*
    if (c->learner_version == 7) return c->scratch != nullptr;                       // SAC: the draws' block
    // TD3: the scratch block, and the trees when the replay is prioritized
    return c->scratch && c->num_batch_reuse == 1 &&
           (!c->prioritized || (c->per_sum && c->per_min && c->per_stamp && c->per_capacity >= c->ring_capacity && c->per_max_priority && c->b_weights));
}

// the driver's first act is the worker's sample on the REAL env, which this model does not have
int real_env_refusal(const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c->cfg.env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM,
                "mpg_step_begin: the real InvertedDoublePendulum-v2 env is MuJoCo and is not provided, so the native step driver (which "
                "samples it) does not serve this model; use the rollout entry points (NADPLearner) on caller-supplied batches");
    return MPG_OK;
}

// ---- AMPC (learner_version 8): what mpg_ampc_pg would refuse of (cfg, batch, M, n), said under the caller's name BEFORE the sample runs ----
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

// everything mpg_step_begin refuses of an AMPC context, each with its own text, before anything is enqueued or any counter moves
int ampc_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c->num_agent > 0 && c->batch > 0 && c->world_size > 0 && c->sampling_interval > 0 && c->ring_capacity > 0,
                "%s: incomplete context (learner_version 8: num_agent %d, batch %d, world_size %d, sampling_interval %d, ring_capacity %d "
                "must all be positive)", entry, c->num_agent, c->batch, c->world_size, c->sampling_interval, c->ring_capacity);
    TRY(real_env_refusal(c));
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

// ---- worker.sample + replay_buffer.add_batch (optimizer.py:332-337, worker.py:91-119) ----
// worker.py:95-112 as one launch (mpg_worker_step): path-tracking env, six-entry observations.  mpg_worker_step serves obs_dim 7 .. 16
// too; the driver does not take it there: its step time against the two launches at K = 3 / 10 has NOT been measured
inline bool worker_step_fused(const mpg_train_ctx_t* c) {
    return c->cfg.env_kind == MPG_ENV_PATH_TRACKING && c->cfg.obs_dim == 6 && c->cfg.act_dim == 2;
}

// worker.py:91-119, the iterations of one sample, as one launch (mpg_worker_rollout) instead of one mpg_worker_step each.  The rule
// for taking it: per width, its median at or below the chain's at both measured sizes (tools/bench_worker_rollout.py).
// A caller that passes sample_iters < 0 asks for |sample_iters| iterations on the chain (include/mpg_hip.h): the A/B switch of that
// measurement and of tests/test_worker_rollout_gpu.py, which compares the two drivers bit for bit.
inline bool worker_rollout_taken(const mpg_train_ctx_t* c) { return c->cfg.obs_dim == 6 && c->sample_iters > 0; }
inline int sample_iters_of(const mpg_train_ctx_t* c) { return c->sample_iters < 0 ? -c->sample_iters : c->sample_iters; }
// the same for the pendulum's real env (mpg_worker_rollout_pendulum instead of mpg_policy_action + mpg_env_step_store_reset per
// iteration), under the same rule (tools/bench_worker_rollout.py --env pendulum) and with the same A/B switch
inline bool pendulum_rollout_taken(const mpg_train_ctx_t* c) {
    return c->cfg.env_kind == MPG_ENV_INVERTED_PENDULUM && c->cfg.obs_dim == 4 && c->cfg.act_dim == 1 && c->sample_iters > 0;
}

// MPGLearner.sample on the pendulum (learner_version 1: the n real-env steps from the replay batch behind the n-step target) as one
// launch (mpg_env_rollout_pendulum) instead of mpg_env_reset_from_obs + n x (mpg_policy_action, mpg_env_step), under the same rule
// (tools/bench_env_rollout_pendulum.py) and with the same A/B switch: sample_iters < 0 keeps this chain too
inline bool env_rollout_pendulum_taken(const mpg_train_ctx_t* c) { return c->sample_iters > 0; }

// what the loop of sample_and_add does behind each of the k iterations a one-launch sample has just run: the counters, and the new
// transitions' priorities and the ring position in iteration order
int rollout_added(mpg_train_ctx_t* c, int k, mpg_stream_t s) {
    const int n = c->num_agent;
    c->noise_ctr += k;
    c->env_ctr += k;
    for (int it = 0; it < k; ++it) {
        // new transitions enter at the max priority (buffer.py:127-136), in iteration order: mpg_per_add reads no ring row and
        // the worker's launch reads no tree
        if (c->learner_version == 4 && c->prioritized)
            TRY(mpg_per_add(c->per_sum, c->per_min, c->per_stamp, c->per_capacity, c->ring_capacity, c->ring_next, n, c->per_alpha,
                            c->per_max_priority, reinterpret_cast<int*>(c->scratch), s));
        c->ring_next = (c->ring_next + n) % c->ring_capacity;
        c->ring_size = std::min(c->ring_size + n, c->ring_capacity);
    }
    return MPG_OK;
}

// draws_now: MPG-v2 draws its minibatch right after the add.  The last env launch then gathers it in spare workgroups (the random
// ring reads overlap the env's sub-steps) except the rows drawn from the slots that launch is writing (path-tracking env, six-entry
// observations); *pre_gathered and *fresh_start tell the gradient launch so (written only then; NADP and TD3 pass draws_now = false).
int sample_and_add(mpg_train_ctx_t* c, const float* policy, bool draws_now, bool* pre_gathered, int* fresh_start, mpg_stream_t s) {
    const int od = c->cfg.obs_dim, kind = c->cfg.env_kind, sample_iters = sample_iters_of(c);
    int it = 0;
    // The iterations before the one that pre-gathers the draw as ONE launch (mpg_worker_rollout: bit-identical to the loop below) when
    // there are at least two of them (and at most the 1024 that launch takes) and the ring holds them all (iters * n <= capacity is what
    // that launch asks: no slot written twice).  With one iteration - num_agent == batch, the benchmark's configuration - nothing changes.
    {
        const bool last_predraws = draws_now && kind == MPG_ENV_PATH_TRACKING && od == 6;
        const int k = sample_iters - (last_predraws ? 1 : 0);
        if (k >= 2 && k <= 1024 && (long)k * c->num_agent <= c->ring_capacity && worker_step_fused(c) && worker_rollout_taken(c)) {
            const int n = c->num_agent;
            TRY(mpg_worker_rollout(&c->cfg, policy, n, k, c->env_state, c->w_obs, c->explore_sigma, c->worker_seed, c->noise_ctr, c->w_act,
                                   c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                   c->env_seed, c->env_ctr, c->w_done, s));
            TRY(rollout_added(c, k, s));
            it = k;
        }
    }
    // The pendulum's sample as ONE launch (mpg_worker_rollout_pendulum: bit-identical to the two launches per iteration of the loop
    // below) under the same conditions; no iteration pre-gathers a draw on this env, so the launch takes them all.
    if (pendulum_rollout_taken(c) && sample_iters >= 2 && sample_iters <= 1024 && (long)sample_iters * c->num_agent <= c->ring_capacity) {
        TRY(mpg_worker_rollout_pendulum(&c->cfg, policy, c->num_agent, sample_iters, c->env_state, c->w_obs, c->explore_sigma, c->worker_seed,
                                        c->noise_ctr, c->w_act, c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew,
                                        c->ring_obs2, c->ring_done, c->env_seed, c->env_ctr, c->w_done, s));
        TRY(rollout_added(c, sample_iters, s));
        it = sample_iters;
    }
    for (; it < sample_iters; ++it) {
        MPG_REQUIRE(c->num_agent <= c->ring_capacity, "mpg_step_begin: ring smaller than one sample");
        const bool predraw = draws_now && it == sample_iters - 1 && kind == MPG_ENV_PATH_TRACKING && od == 6;
        mpg_replay_draw_t pd = {};
        if (predraw) {
            pd.n_storage = std::min(c->ring_size + c->num_agent, c->ring_capacity);
            pd.seed = c->replay_seed; pd.ctr = c->replay_times + 1;
            pd.idx_out = c->idx; pd.done_out = c->b_done;
            *pre_gathered = true;
            *fresh_start = c->ring_next;
        }
        if (worker_step_fused(c)) {
            // the policy pass, env.step -> ring slot (next + i) % capacity -> env.reset of the done agents (and the draw): one launch
            TRY(mpg_worker_step(&c->cfg, policy, c->num_agent, c->env_state, c->w_obs, c->explore_sigma, c->worker_seed, c->noise_ctr++,
                                c->w_act, c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                c->env_seed, c->env_ctr++, c->w_done, predraw ? &pd : nullptr, c->batch, c->b_obs, c->b_act, c->b_rew,
                                c->b_obs2, s));
        } else {
            TRY(mpg_policy_action(&c->cfg, policy, c->num_agent, c->w_obs, c->explore_sigma, c->worker_seed, c->noise_ctr++, c->w_act, s));
            // env.step -> ring slot (next + i) % capacity -> env.reset of the done agents, one launch
            mpg_prof_begin(c->cfg.prof, 2, mpg_stream(s));
            if (predraw) {
                TRY(mpg_env_step_store_reset_draw(kind, c->num_agent, od, c->env_state, c->w_act, c->ring_capacity, c->ring_next,
                                                  c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done, c->env_seed,
                                                  c->env_ctr++, c->w_obs, c->w_done, &pd, c->batch, c->b_obs, c->b_act, c->b_rew,
                                                  c->b_obs2, s));
            } else {
                TRY(mpg_env_step_store_reset(kind, c->num_agent, od, c->env_state, c->w_act, c->ring_capacity, c->ring_next, c->ring_obs,
                                             c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done, c->env_seed, c->env_ctr++, c->w_obs,
                                             c->w_done, s));
            }
            mpg_prof_end(c->cfg.prof, 2, mpg_stream(s));
        }
        if (c->learner_version == 4 && c->prioritized)       // new transitions enter at the max priority (buffer.py:127-136)
            TRY(mpg_per_add(c->per_sum, c->per_min, c->per_stamp, c->per_capacity, c->ring_capacity, c->ring_next, c->num_agent,
                            c->per_alpha, c->per_max_priority, reinterpret_cast<int*>(c->scratch), s));
        c->ring_next = (c->ring_next + c->num_agent) % c->ring_capacity;
        c->ring_size = std::min(c->ring_size + c->num_agent, c->ring_capacity);
    }
    return MPG_OK;
}

// ---- NADPLearner.compute_gradient, learners/nadp.py:209-241 (networks [Q1 | policy]) ----
int nadp_gradients(mpg_train_ctx_t* c, const Layout& l, mpg_stream_t s) {
    const float* q1 = c->params;
    const float* policy = c->params + l.off[1];
    const float* q1t = c->targets;
    const float inv_b = 1.f / ((float)c->batch * (float)c->world_size);
    float* stats = c->grad + l.n_grad;
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
int td3_gradients(mpg_train_ctx_t* c, const Layout& l, mpg_stream_t s) {
    const int ad = c->cfg.act_dim, B = c->batch;
    const float *q1 = c->params, *q2 = c->params + l.off[1], *policy = c->params + l.off[2];
    const float *q1t = c->targets, *q2t = c->targets + l.off[1], *policy_t = c->targets + l.off[2];
    const float inv_b = 1.f / ((float)B * (float)c->world_size);
    float* stats = c->grad + l.n_grad;
    float* eps = c->scratch;                          // [B][ad] smoothing noise
    float* y1 = eps + (size_t)B * ad;                 // [B] the priorities' plain Q1 target
    float* td = y1 + B;                               // [B] Q1(s, a) - y
    float* perr = td + B;                             // [B] y1 - Q1(s, a)
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
//      (:57-72,127-151) every num_batch_reuse-th call ----
int ndpg_gradients(mpg_train_ctx_t* c, const Layout& l, bool fresh, mpg_stream_t s) {
    const int od = c->cfg.obs_dim, ad = c->cfg.act_dim;
    const float* q1 = c->params;
    const float* policy = c->params + l.off[1];
    const float inv_b = 1.f / ((float)c->batch * (float)c->world_size);
    float* stats = c->grad + l.n_grad;
    if (fresh) {
        TRY(mpg_replay_sample_uniform(c->ring_size, c->batch, c->replay_seed, c->replay_times, od, ad, c->ring_obs, c->ring_act,
                                      c->ring_rew, c->ring_obs2, c->ring_done, c->idx, c->b_obs, c->b_act, c->b_rew, c->b_obs2,
                                      c->b_done, s));
        TRY(mpg_env_rollout(&c->cfg, policy, c->batch, c->n, c->b_obs, c->b_act, c->l_rewards, c->l_obs, s));
        TRY(mpg_nstep_targets(&c->cfg, c->targets + l.off[1], c->targets, c->batch, c->n, c->l_rewards, c->l_obs, c->b_targets, c->ws0,
                              c->ws0_bytes, s));
    }
    TRY(mpg_q_loss_grad(&c->cfg, q1, c->batch, c->b_obs, c->b_act, c->b_targets, inv_b, stats, c->grad + l.off[0], nullptr, c->ws0,
                        c->ws0_bytes, s));
    return mpg_dpg_policy_grad(&c->cfg, policy, q1, c->batch, c->b_obs, inv_b, stats + 2, stats + 3, c->grad + l.off[1], c->ws1,
                               c->ws1_bytes, s);
}

// ---- SAC (learner_version 7): worker.py:68-79 with a stochastic policy + replay_buffer.add_batch ----
// The draw, the policy pass, the Gaussian head, env.step -> ring slot (next + i) % capacity -> env.reset of the done agents: ONE launch
// (mpg_worker_sample_step) at every width.  Against the three calls it replaces (mpg_normal_fill, mpg_policy_sample,
// mpg_env_step_store_reset: four launches, bit-identical) it measured faster at 8 and at 4096 agents with obs_dim 6 and 9
// (tools/bench_sac_native.py), which is the rule for taking it.
//
// A sample's iterations as ONE launch (mpg_worker_sample_rollout: bit-identical to the loop of mpg_worker_sample_step calls) under
// sample_and_add's conditions - at least two iterations, at most the 1024 that launch takes, the ring holds them all - and its rule
// per width (tools/bench_worker_rollout.py --stochastic); sample_iters < 0 keeps the chain, as there.
inline bool sac_rollout_taken(const mpg_train_ctx_t* c) { return c->sample_iters > 0; }

int sac_sample_and_add(const char* entry, mpg_train_ctx_t* c, const float* policy, mpg_stream_t s) {
    const int n = c->num_agent, sample_iters = sample_iters_of(c);
    MPG_REQUIRE(n <= c->ring_capacity, "%s: ring smaller than one sample", entry);
    int it = 0;
    if (sac_rollout_taken(c) && sample_iters >= 2 && sample_iters <= 1024 && (long)sample_iters * n <= c->ring_capacity) {
        TRY(mpg_worker_sample_rollout(&c->cfg, policy, n, sample_iters, c->env_state, c->w_obs, c->worker_seed, c->noise_ctr, c->w_act,
                                      c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                      c->env_seed, c->env_ctr, c->w_done, s));
        TRY(rollout_added(c, sample_iters, s));            // (learner_version 7: the counters and the ring position)
        it = sample_iters;
    }
    for (; it < sample_iters; ++it) {
        // (the log-densities have no consumer: worker.py:96 drops them)
        TRY(mpg_worker_sample_step(&c->cfg, policy, n, c->env_state, c->w_obs, c->worker_seed, c->noise_ctr++, c->w_act, nullptr,
                                   c->ring_capacity, c->ring_next, c->ring_obs, c->ring_act, c->ring_rew, c->ring_obs2, c->ring_done,
                                   c->env_seed, c->env_ctr++, c->w_done, s));
        c->ring_next = (c->ring_next + n) % c->ring_capacity;
        c->ring_size = std::min(c->ring_size + n, c->ring_capacity);
    }
    return MPG_OK;
}

// ---- SACLearner.compute_gradient, learners/sac.py:169-219 (networks [Q1 | Q2 | policy]); the minibatch and its soft target
//      (:67-80) every num_batch_reuse-th call.  Draws: counters 2 (k + 1) for the target of call k, 2 k + 1 for the policy loss after
//      the counter's increment, as SACLearner._draw.
//      at non-null: the learned temperature - alpha is read on the device (at->state), the _auto entry points run, the third draw (stream
//      learner_seed + 2, the counter after its increment) goes into the second half of the scratch block, the temperature's gradient
//      into grad[n_grad] and the statistics one float further on: [grads | alpha grad | stats] ----
int sac_gradients(mpg_train_ctx_t* c, const Layout& l, float alpha, const mpg_sac_alpha_t* at, bool fresh, mpg_stream_t s) {
    const int od = c->cfg.obs_dim, ad = c->cfg.act_dim, B = c->batch;
    const float *q1 = c->params, *q2 = c->params + l.off[1], *policy = c->params + l.off[2];
    const float *q1t = c->targets, *q2t = c->targets + l.off[1];
    const float inv_b = 1.f / ((float)B * (float)c->world_size);
    float* stats = c->grad + l.n_grad + (at ? 1 : 0);
    float* eps = c->scratch;                          // [B][ad]
    if (fresh) {
        TRY(mpg_replay_sample_uniform(c->ring_size, B, c->replay_seed, c->replay_times, od, ad, c->ring_obs, c->ring_act, c->ring_rew,
                                      c->ring_obs2, c->ring_done, c->idx, c->b_obs, c->b_act, c->b_rew, c->b_obs2, c->b_done, s));
        TRY(mpg_normal_fill(B * ad, c->learner_seed, 2 * (c->learner_counter + 1), eps, s));
        if (at)
            TRY(mpg_sac_targets_auto(&c->cfg, policy, q1t, q2t, B, c->b_rew, c->b_obs2, eps, at->state, c->b_targets, c->ws0, c->ws0_bytes, s));
        else
            TRY(mpg_sac_targets(&c->cfg, policy, q1t, q2t, B, c->b_rew, c->b_obs2, eps, alpha, c->b_targets, c->ws0, c->ws0_bytes, s));
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
    return mpg_sac_policy_grad(&c->cfg, policy, q1, q2, B, c->b_obs, eps, alpha, inv_b, stats + 2, stats + 3, stats + 4, c->grad + l.off[2],
                               c->ws1, c->ws1_bytes, s);
}

// ---- AMPCLearner.compute_gradient, learners/ampc.py:105-122 (networks [policy]): the statistics are the two return sums; the noise
//      counter is the one AMPCLearner uses after _begin has counted the call ----
int ampc_gradients(mpg_train_ctx_t* c, const Layout& l, mpg_stream_t s) {
    const float inv_b = 1.f / ((float)c->batch * (float)c->world_size);
    float* stats = c->grad + l.n_grad;
    return mpg_ampc_pg(&c->cfg, c->params, c->batch, c->M, c->n, c->b_obs, nullptr, c->learner_seed, 2 * c->learner_counter + 1, inv_b, stats,
                       stats + 1, c->grad, c->ws1, c->ws1_bytes, s);
}

}  // namespace

extern "C" int mpg_step_workspace_bytes(const mpg_train_ctx_t* c, size_t* ws0, size_t* ws1) {
    MPG_REQUIRE(c && ws0 && ws1, "mpg_step_workspace_bytes: null pointer");
    MPG_REQUIRE((c->learner_version >= 1 && c->learner_version <= 5) || c->learner_version == 7 || c->learner_version == 8,
                "mpg_step_workspace_bytes: unknown learner_version %d", c->learner_version);
    if (is_ampc(c)) {                    // AMPC: no target and no critic; the rollout gradient
        TRY(ampc_shape_refusal("mpg_step_workspace_bytes", c));
        *ws0 = 0;
        *ws1 = mpg_ampc_pg_workspace_bytes(&c->cfg, c->batch, c->M, c->n);
        return MPG_OK;
    }
    if (c->learner_version == 7) {       // SAC: soft targets / critic loss; the Gaussian-head policy gradient
        *ws0 = std::max(mpg_sac_targets_workspace_bytes(&c->cfg, c->batch), mpg_q_loss_grad_workspace_bytes(&c->cfg, c->batch));
        *ws1 = mpg_sac_policy_grad_workspace_bytes(&c->cfg, c->batch);
        MPG_REQUIRE(*ws0 && *ws1, "mpg_step_workspace_bytes: unsupported configuration");
        return MPG_OK;
    }
    *ws0 = std::max(mpg_q_targets_workspace_bytes(&c->cfg, c->batch), mpg_q_loss_grad_workspace_bytes(&c->cfg, c->batch));
    if (c->learner_version == 3) {
        *ws0 = std::max(*ws0, mpg_rollout_q_target_workspace_bytes(&c->cfg, c->batch));
        *ws1 = mpg_rollout_pg_workspace_bytes(&c->cfg, c->batch, 1, c->n, 2, 1);
    } else if (c->learner_version == 4) {
        *ws1 = mpg_td3_policy_grad_workspace_bytes(&c->cfg, c->batch);
    } else if (c->learner_version == 5) {
        *ws1 = mpg_dpg_policy_grad_workspace_bytes(&c->cfg, c->batch);
    } else
    *ws1 = mpg_mpg_gradients_workspace_bytes(&c->cfg, c->batch, c->M, c->n, c->n_select, c->learner_version == 2 ? 2 : 1);
    MPG_REQUIRE(*ws0 && *ws1, "mpg_step_workspace_bytes: unsupported configuration");
    return MPG_OK;
}

extern "C" int mpg_step_begin(mpg_train_ctx_t* c, int iteration, mpg_stream_t s) {
    MPG_REQUIRE(!c || c->learner_version != 7,
                "mpg_step_begin: learner_version 7 (SAC) takes its temperature as an argument: call mpg_sac_step_begin");
    if (c && is_ampc(c)) TRY(ampc_refusal("mpg_step_begin", c));      // each refusal in its own words; ctx_ok then holds
    MPG_REQUIRE(ctx_ok(c), "mpg_step_begin: incomplete context");
    TRY(real_env_refusal(c));                                       // refused before anything is enqueued
    const Layout l = layout(c);
    const int od = c->cfg.obs_dim, ad = c->cfg.act_dim, kind = c->cfg.env_kind;
    const float* policy = c->params + l.off[l.n_nets - 1];
    const float* policy_t = c->targets + l.off[l.n_nets - 1];
    if (!is_mpg(c)) {        // ---- NADP / TD3 / NDPG / AMPC: sample, add, replay, gradients (optimizer.py:330-353) ----
        if (iteration % c->sampling_interval == 0) TRY(sample_and_add(c, policy, false, nullptr, nullptr, s));
        MPG_REQUIRE(c->ring_size > 0, "mpg_step_begin: empty replay ring");
        c->replay_times++;
        if (c->learner_version == 5) {       // the batch is drawn on every num_batch_reuse-th call only (ndpg.py:203-204)
            const bool fresh = c->learner_counter % c->num_batch_reuse == 0;
            c->learner_counter++;
            return ndpg_gradients(c, l, fresh, s);
        }
        if (c->learner_version == 4 && c->prioritized) {
            TRY(mpg_per_sample_gather(c->per_sum, c->per_min, c->per_capacity, c->ring_size, c->batch, nullptr, c->replay_seed,
                                      c->replay_times, c->per_beta, c->idx, c->b_weights, od, ad, c->ring_obs, c->ring_act, c->ring_rew,
                                      c->ring_obs2, c->ring_done, c->b_obs, c->b_act, c->b_rew, c->b_obs2, c->b_done, s));
        } else {
            TRY(mpg_replay_sample_uniform(c->ring_size, c->batch, c->replay_seed, c->replay_times, od, ad, c->ring_obs, c->ring_act,
                                          c->ring_rew, c->ring_obs2, c->ring_done, c->idx, c->b_obs, c->b_act, c->b_rew, c->b_obs2,
                                          c->b_done, s));
        }
        c->learner_counter++;
        if (is_ampc(c)) return ampc_gradients(c, l, s);
        return c->learner_version == 3 ? nadp_gradients(c, l, s) : td3_gradients(c, l, s);
    }
    // ---- worker.sample + replay_buffer.add_batch; MPG-v2 draws its minibatch right after the add ----
    const bool draws_now = c->learner_version == 2 && c->learner_counter % c->num_batch_reuse == 0;
    bool pre_gathered = false;
    int fresh_start = 0;
    if (iteration % c->sampling_interval == 0) TRY(sample_and_add(c, policy, draws_now, &pre_gathered, &fresh_start, s));
    // ---- replay_buffer.replay (optimizer.py:340-341; buffer.py:70-91) ----
    MPG_REQUIRE(c->ring_size > 0, "mpg_step_begin: empty replay ring");
    c->replay_times++;
    mpg_replay_draw_t draw = {};
    bool draw_in_gradients = false;
    if (c->learner_counter % c->num_batch_reuse == 0) {       // get_batch_data, mpg_learner.py:402-403
        if (c->learner_version == 2) {
            // the minibatch draw and the clipped double-Q target both ride in the first launch of mpg_mpg_gradients
            draw.n_storage = c->ring_size; draw.seed = c->replay_seed; draw.ctr = c->replay_times;
            draw.ring_obs = c->ring_obs; draw.ring_act = c->ring_act; draw.ring_rew = c->ring_rew; draw.ring_obs2 = c->ring_obs2;
            draw.ring_done = c->ring_done; draw.idx_out = c->idx; draw.done_out = c->b_done;
            draw.pre_gathered = pre_gathered ? 1 : 0; draw.capacity = c->ring_capacity; draw.fresh_start = fresh_start;
            draw.fresh_count = pre_gathered ? c->num_agent : 0;
            draw_in_gradients = true;
        } else {   // MPGLearner.sample + compute_n_step_target, mpg_learner.py:109-124,146-169
            TRY(mpg_replay_sample_uniform(c->ring_size, c->batch, c->replay_seed, c->replay_times, od, ad, c->ring_obs, c->ring_act,
                                          c->ring_rew, c->ring_obs2, c->ring_done, c->idx, c->b_obs, c->b_act, c->b_rew, c->b_obs2,
                                          c->b_done, s));
            MPG_REQUIRE(c->l_env_state && c->l_obs && c->l_act && c->l_rewards && c->l_done, "mpg_step_begin: MPG-v1 needs the learner env buffers");
            // one launch (mpg_env_rollout, bit-identical to the chain below: rewards, last observations, status word) where that entry
            // point serves the configuration; the learner's env state, action and done buffers are not written then
            const bool ranged_tanh = c->cfg.policy_out_act == MPG_ACT_TANH && c->cfg.action_range > 0.f;
            const bool pendulum = kind == MPG_ENV_INVERTED_PENDULUM;
            const bool one_launch = kind == MPG_ENV_PATH_TRACKING && ad == 2 && c->n < 32 && !ranged_tanh;
            // the pendulum's one launch (mpg_env_rollout_pendulum, bit-identical to the chain too) for the horizons it serves, by the
            // rule of the worker's one-launch samples (env_rollout_pendulum_taken, above); longer horizons keep the chain
            const bool one_launch_pendulum = pendulum && od == 4 && ad == 1 && c->n <= 1024 && !ranged_tanh && env_rollout_pendulum_taken(c);
            if (one_launch) TRY(mpg_env_rollout(&c->cfg, policy, c->batch, c->n, c->b_obs, c->b_act, c->l_rewards, c->l_obs, s));
            else if (one_launch_pendulum)
                TRY(mpg_env_rollout_pendulum(&c->cfg, policy, c->batch, c->n, c->b_obs, c->b_act, c->l_rewards, c->l_obs, s));
            else TRY(mpg_env_reset_from_obs(kind, c->batch, od, c->l_env_state, c->b_obs, s));
            for (int t = 0; t < c->n && !one_launch && !one_launch_pendulum; ++t) {
                const float* act = c->b_act;
                if (t > 0) {
                    TRY(mpg_policy_action(&c->cfg, policy, c->batch, c->l_obs, 0.f, 0, 0, c->l_act, s));
                    act = c->l_act;
                }
                TRY(mpg_env_step(kind, c->batch, od, c->l_env_state, act, c->l_obs, c->l_rewards + (size_t)t * c->batch, c->l_done,
                                 c->l_done_intended, s));
            }
            // the pendulum's bootstrap value is clipped (mpg_learner.py:163-164), whichever way the rollout was taken
            if (pendulum)
                TRY(mpg_nstep_targets_clipped(&c->cfg, policy_t, c->targets + l.off[0], c->batch, c->n, c->l_rewards, c->l_obs,
                                              MPG_PENDULUM_NSTEP_Q_LO, MPG_PENDULUM_NSTEP_Q_HI, c->b_targets, c->ws0, c->ws0_bytes, s));
            else
                TRY(mpg_nstep_targets(&c->cfg, policy_t, c->targets + l.off[0], c->batch, c->n, c->l_rewards, c->l_obs, c->b_targets,
                                      c->ws0, c->ws0_bytes, s));
        }
    }
    c->learner_counter++;
    // ---- learner.compute_gradient (mpg_learner.py:401-431), un-clipped partials scaled by 1/B_global ----
    const float inv_b = 1.f / ((float)c->batch * (float)c->world_size);
    float w[4];
    rule_based_weights(iteration, c->total_ite, c->eta, c->select, c->n_select, w);
    // MPG-v2 with num_batch_reuse > 1 keeps the targets of the batch they were computed for (mpg_learner.py:402-403)
    const bool fresh = (c->learner_counter - 1) % c->num_batch_reuse == 0;
    const float* y_in = (c->learner_version == 2 && fresh) ? nullptr : c->b_targets;
    // scheduling option (include/mpg_hip.h, mpg_grad_opts_t): with an exchange and the caller's event, the critics' gradient is finished
    // ahead of the reverse sweep
    c->grad_opts.critics_ready_event = exchanged(c) ? c->critics_ready_event : nullptr;
    c->cfg.grad_opts = &c->grad_opts;
    const int rc = mpg_mpg_gradients(&c->cfg, l.n_nets - 1, c->params, c->targets, c->batch, c->b_obs, c->b_act, c->b_rew, c->b_obs2, y_in,
                                     c->M, c->n, c->select, c->n_select, w, nullptr, c->learner_seed, c->learner_counter, inv_b, c->grad,
                                     c->grad + l.n_grad, c->b_targets, exchanged(c) ? nullptr : c->clip_scratch,
                                     draw_in_gradients ? &draw : nullptr, c->ws1, c->ws1_bytes, s);
    c->cfg.grad_opts = nullptr;
    return rc;
}

namespace {
// what mpg_sac_step_begin and mpg_sac_auto_step_begin refuse alike, under the caller's name
int sac_begin_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c, "%s: null context", entry);
    MPG_REQUIRE(c->learner_version == 7, "%s: learner_version 7 (SAC) only (got %d)", entry, c->learner_version);
    MPG_REQUIRE(ctx_ok(c), "%s: incomplete context", entry);
    MPG_REQUIRE(!c->prioritized, "%s: a prioritized replay buffer is not served (prioritized = %d)", entry, c->prioritized);
    MPG_REQUIRE(c->explore_sigma == 0.f, "%s: explore_sigma on top of the stochastic policy is not served (got %g)", entry,
                (double)c->explore_sigma);
    return MPG_OK;
}
int sac_begin_env_refusal(const char* entry, const mpg_train_ctx_t* c) {
    MPG_REQUIRE(c->cfg.env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM,
                "%s: the real InvertedDoublePendulum-v2 env is MuJoCo and is not provided, so the native step driver (which "
                "samples it) does not serve this model", entry);
    return MPG_OK;
}
int sac_begin(const char* entry, mpg_train_ctx_t* c, float alpha, const mpg_sac_alpha_t* at, int iteration, mpg_stream_t s) {
    const Layout l = layout(c);
    if (iteration % c->sampling_interval == 0) TRY(sac_sample_and_add(entry, c, c->params + l.off[2], s));
    MPG_REQUIRE(c->ring_size > 0, "%s: empty replay ring", entry);
    c->replay_times++;
    const bool fresh = c->learner_counter % c->num_batch_reuse == 0;     // the batch is drawn on every num_batch_reuse-th call only
    return sac_gradients(c, l, alpha, at, fresh, s);
}
}  // namespace

extern "C" int mpg_sac_step_begin(mpg_train_ctx_t* c, float alpha, int iteration, mpg_stream_t s) {
    TRY(sac_begin_refusal("mpg_sac_step_begin", c));
    MPG_REQUIRE(alpha >= 0.f && alpha <= 3.4028234664e38f, "mpg_sac_step_begin: alpha must be finite and not negative (got %g)",
                (double)alpha);
    TRY(sac_begin_env_refusal("mpg_sac_step_begin", c));
    return sac_begin("mpg_sac_step_begin", c, alpha, nullptr, iteration, s);
}

extern "C" int mpg_sac_auto_step_begin(mpg_train_ctx_t* c, const mpg_sac_alpha_t* a, int iteration, mpg_stream_t s) {
    TRY(sac_begin_refusal("mpg_sac_auto_step_begin", c));
    MPG_REQUIRE(a, "mpg_sac_auto_step_begin: null temperature struct");
    MPG_REQUIRE(a->state, "mpg_sac_auto_step_begin: null temperature state");
    MPG_REQUIRE(std::isfinite(a->target_entropy), "mpg_sac_auto_step_begin: target_entropy must be finite (got %g)", (double)a->target_entropy);
    TRY(sac_begin_env_refusal("mpg_sac_auto_step_begin", c));
    return sac_begin("mpg_sac_auto_step_begin", c, 0.f, a, iteration, s);
}

extern "C" int mpg_step_end(mpg_train_ctx_t* c, int iteration, mpg_stream_t s) {
    MPG_REQUIRE(ctx_ok(c) && c->norms && c->nonfinite && c->adam_m && c->adam_v && c->clip_scratch, "mpg_step_end: incomplete context");
    const Layout l = layout(c);
    // per-network clip_by_global_norm (mpg_learner.py:415-431): on one GPU the partial sums of squares were left in
    // clip_scratch by mpg_mpg_gradients; after an all-reduce they are recomputed from the reduced gradient
    // (NADP / TD3: their gradient launches leave no partials, they are always taken from the gradient buffer); an exchange that
    // sums with mpg_sum_slots_sq has left them already (clip_partials_ready)
    if ((exchanged(c) && !c->clip_partials_ready) || (!exchanged(c) && !is_mpg(c))) TRY(mpg_sq_partials(c->grad, l.sizes, l.n_nets, c->clip_scratch, s));
    // PolicyWithQs.apply_gradients, policy.py:123-156
    // (AMPC: a policy-only stack has no delay and no target, policy.py:125-127 - delay_update and tau are not looked at)
    const bool delayed = is_ampc(c) || iteration % c->delay_update == 0;
    float lr_t[3];
    int do_adam[3], do_polyak[3];
    for (int k = 0; k < l.n_nets; ++k) {
        const bool is_policy = k == l.n_nets - 1;
        const bool upd = !is_policy || delayed;
        const long long t = c->opt_steps[k] + 1;
        lr_t[k] = adam_step_size(is_policy ? c->policy_lr : c->value_lr, c->opt_steps[k]);
        do_adam[k] = upd ? 1 : 0;
        do_polyak[k] = delayed && !is_ampc(c) ? 1 : 0;
        if (upd) c->opt_steps[k] = t;
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
    MPG_REQUIRE(c->learner_version == 7, "mpg_sac_auto_step_end: learner_version 7 (SAC) only (got %d)", c->learner_version);
    MPG_REQUIRE(a, "mpg_sac_auto_step_end: null temperature struct");
    MPG_REQUIRE(a->state, "mpg_sac_auto_step_end: null temperature state");
    MPG_REQUIRE(ctx_ok(c) && c->norms && c->nonfinite && c->adam_m && c->adam_v && c->clip_scratch, "mpg_sac_auto_step_end: incomplete context");
    MPG_REQUIRE(c->clip > 0.f && a->opt_steps >= 0, "mpg_sac_auto_step_end: clip norm %g / temperature step counter %lld", (double)c->clip,
                a->opt_steps);
    const Layout l = layout(c);
    TRY(mpg_step_end(c, iteration, s));
    return mpg_sac_alpha_update(a, c->grad + l.n_grad, c->clip, 1, iteration % c->delay_update == 0 ? 1 : 0, c->nonfinite, l.n_nets, s);
}
