// Host-side glue shared by the C-ABI entry points (learner_api.hip, rollout_kernels.hip, rollout_common.h): the workspace arena,
// the configuration predicates and the network input / output descriptions of a cfg.  Internal to libmpg_hip.so.
#pragma once
#include "mlp_launch.h"

namespace mlp {

// A caller-owned workspace as a sequence of 256-byte aligned arrays.  ONE function per workspace names its arrays in order; run on a
// measuring arena (no buffer) it yields the `*_workspace_bytes` answer, run on the caller's buffer it yields the arrays, and fits()
// says whether they lie inside it - the same code, so the size a query reports and the carve behind it cannot disagree.
// Every array is charged its bytes rounded up to 256 plus 256: that covers the alignment of an unaligned buffer, and the rest is
// slack behind each array.
// Shown (tests/test_workspace_guard_gpu.py, both engines, every entry point that takes a workspace, at row counts with dead rows in a
// group, a short last weight-gradient chunk and fewer thin partials than the array holds): the entry points run in exactly the queried
// size, from a 256-byte aligned buffer and from one 4 bytes off such a line; they write nothing outside it (1 MiB guards on either side
// stay intact); and their results do not depend on what it held - bit-identical after 0xFF bytes (every float a NaN) and after zeros,
// although a call leaves part of the words unwritten (the test prints how many).  The kernels write whatever they read: there is no
// memset here to rely on.
// Not shown: that the kernels' clamped / wide loads and stores can do without the 256 bytes behind each array - a write into that slack
// lies inside the workspace, where guards at its two ends cannot see it.
struct Arena {
    uintptr_t p;            // next array (0: measuring)
    size_t have, need = 0;
    Arena() : p(0), have(0) {}
    Arena(void* ws, size_t bytes) : p((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255)), have(bytes) {}
    void* bytes(size_t n) {
        n = (n + 255) & ~size_t(255);
        need += n + 256;
        void* r = reinterpret_cast<void*>(p);
        if (p) p += n;
        return r;
    }
    float* take(size_t nfloat) { return static_cast<float*>(bytes(nfloat * sizeof(float))); }
    bool fits() const { return need <= have; }
};

// the `*_workspace_bytes` answer of a workspace description: what it takes from an arena without a buffer
template <class F, class... A>
size_t measured(F describe, A... args) {
    Arena ar;
    describe(ar, args...);
    return ar.need;
}

// the one refusal of a workspace (checked before anything is enqueued)
inline int workspace_too_small(const char* entry, size_t have, size_t need) {
    mpg_set_error("%s: workspace too small (%zu < %zu)", entry, have, need);
    return MPG_EWORKSPACE;
}

// the network shapes that are built, and an output activation the kernels implement
inline bool net_cfg_ok(const mpg_cfg_t* c) {
    // policy_out_activation='tanh' WITH an action_range would be range*tanh(tanh(z)) in the reference (policy.py:176-177,
    // 197-199); the kernels implement range*tanh(z) / tanh(z) / z only, so that combination is refused, not approximated
    // (obs 11, act 1: the double pendulum's observation, include/mpg_hip.h MPG_ENV_INVERTED_DOUBLE_PENDULUM)
    return c && ((c->obs_dim >= 6 && c->obs_dim <= 16 && c->act_dim == 2) || ((c->obs_dim == 4 || c->obs_dim == 11) && c->act_dim == 1)) &&
           !(c->policy_out_act == MPG_ACT_TANH && c->action_range > 0.f);
}
// ... and the model of the rollout is the one those shapes belong to
inline bool rollout_cfg_ok(const mpg_cfg_t* c) {
    return net_cfg_ok(c) && c->env_kind == (c->act_dim == 2   ? MPG_ENV_PATH_TRACKING
                                            : c->obs_dim == 4 ? MPG_ENV_INVERTED_PENDULUM
                                                              : MPG_ENV_INVERTED_DOUBLE_PENDULUM);
}

inline OutSpec linear_out() {
    OutSpec o;
    o.out_tanh = 0; o.out_scale = 1.f; o.sigma = 0.f; o.seed = 0; o.ctr = 0;
    return o;
}
inline OutSpec policy_out(const mpg_cfg_t* c) {
    OutSpec o = linear_out();
    const bool ranged = c->action_range > 0.f;
    o.out_tanh = (c->policy_out_act == MPG_ACT_TANH || ranged) ? 1 : 0;
    o.out_scale = ranged ? c->action_range : 1.f;
    return o;
}

// network inputs of a cfg: the policy sees the scaled observation, a critic (scaled observation | action)
inline XSpec policy_x(const mpg_cfg_t* c, const float* obs) { return xspec(obs, c->obs_dim, nullptr, 0, c->obs_scale, c->obs_dim); }
inline XSpec critic_x(const mpg_cfg_t* c, const float* obs, const float* act) {
    return xspec(obs, c->obs_dim, act, c->act_dim, c->obs_scale, c->obs_dim);
}

// act [rows][act_dim] = policy(obs); q [rows] = critic(x); optional G16 stashes (launch_forward)
inline int policy_forward(const mpg_cfg_t* c, const float* params, int rows, const XSpec& x, const OutSpec& o, float* act, float* h1,
                          float* h2, hipStream_t s) {
    return launch_forward(c, params, c->obs_dim, 2 * c->act_dim, c->act_dim, rows, x, o, act, c->act_dim, h1, h2, s);
}
inline int critic_forward(const mpg_cfg_t* c, const float* params, int rows, const XSpec& x, float* q, float* h1, float* h2,
                          hipStream_t s) {
    return launch_forward(c, params, c->obs_dim + c->act_dim, 1, 1, rows, x, linear_out(), q, 1, h1, h2, s);
}

}  // namespace mlp
