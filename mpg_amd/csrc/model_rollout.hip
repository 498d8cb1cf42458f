// The differentiable models on their own: mpg_model_step, one rollout_out of the model a cfg names (k_model_step, one lane per row),
// and mpg_model_rollout, a policy's closed loop on that model in one launch (k_model_rollout) - what mpg_eval_rollout is for the real
// envs, for the models the learners optimise through (rollout_common.h: PathTracking, Pendulum, DoublePendulum), the double pendulum
// included, whose real env does not exist here.
//
// Both kernels live in THIS translation unit under one contraction mode - the block below, the mode the network engine and the sweeps'
// models are compiled under everywhere - and form a row's step by CALLING one function that is not inlined (model_row_call), so that
// the launch and the chain of mpg_policy_action + mpg_model_step it replaces agree bit for bit (what a library
// routine expanded differently in two units cost before; f19: what inlining one body into two kernels of one unit cost here).  The
// model bodies are rollout_common.h's, the policy pass is policy_pass.h's.
#include <type_traits>

#pragma clang fp contract(fast)
#include "rollout_common.h"
#include "policy_pass.h"
#include "env_internal.h"

namespace model_rollout {
using namespace mlp;

constexpr int XW = 16;          // the widest observation row (PathTracking with ten look-ahead entries)
// the leading entries of an observation row that ENV's step READS - what a trajectory lane keeps in registers from step to step
template <class ENV> constexpr int reads() {
    if constexpr (rollout::has_features<ENV>::value) return 8; else return ENV::OBS;
}

// the observation width of ENV's launches: the kind's own, or 0 for "6 .. 16, the cfg's" (PathTracking's 16-wide form)
template <class ENV, int IN> constexpr int fixed_width() {
    if constexpr (rollout::has_features<ENV>::value) return ENV::NFEAT;
    else return std::is_same<ENV, rollout::PathTracking>::value && IN == XW ? 0 : ENV::OBS;
}

// One rollout_out on an observation row's leading entries x: what the forward sweep's chain computes per step -
// ENV::pre + ENV::finish - from the row taken the way the sweeps take a START observation:
//   PathTracking: not wrapped, the look-ahead entries are not read; those of the new row are copies of delta_y (FUT_SRC);
//   Pendulum: the four entries;
//   DoublePendulum: the state is ENV::reset's atan2 of the row's sines and cosines, the new row ENV::features of the new state.
// eps: the standard-normal model noise (the double pendulum has none).  rew is RAW.
// (NOT inlined: the step kernel and the rollout kernel CALL the same instructions.  Inlined into both, the body was contracted
// differently in the two - a reward came out one ulp apart in one row of sixteen - although both sit in this unit under one mode.
// Arguments and results are small structs by value: they travel in registers.)
struct RowIn {
    float x[8], a[2], eps;
};
struct RowOut {
    float x[8], rew;        // the entries of the new row that are not copies or zeros: reads<ENV>() of them
};
template <class ENV>
__device__ __noinline__ RowOut model_row_call(const RowIn in) {
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, on[8], p[ENV::NPRE];
    RowOut out;
    if constexpr (rollout::has_features<ENV>::value) {
        ENV::reset(in.x, o);
        ENV::pre(o, in.eps, p);
        float tr[4], f[ENV::NFEAT];
        ENV::finish(p, in.a, on, out.rew, tr);
        ENV::features(on, tr, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) out.x[k] = f[k];
    } else {
#pragma unroll
        for (int k = 0; k < ENV::OBS; ++k) o[k] = in.x[k];
        ENV::pre(o, in.eps, p);
        ENV::finish(p, in.a, on, out.rew);
#pragma unroll
        for (int k = 0; k < 8; ++k) out.x[k] = on[k];
    }
    return out;
}
template <class ENV>
__device__ __forceinline__ void model_row(const float (&x)[reads<ENV>()], const float (&a)[2], float eps, float (&xn)[XW], float& rew) {
    RowIn in;
#pragma unroll
    for (int k = 0; k < 8; ++k) in.x[k] = k < reads<ENV>() ? x[k < reads<ENV>() ? k : 0] : 0.f;
    in.a[0] = a[0]; in.a[1] = a[1]; in.eps = eps;
    const RowOut out = model_row_call<ENV>(in);
    rew = out.rew;
    // the rest of the new row: PathTracking's look-ahead entries are copies of delta_y, the double pendulum's last three are zeros
#pragma unroll
    for (int k = 0; k < XW; ++k)
        xn[k] = k < reads<ENV>() ? out.x[k < 8 ? k : 0] : (rollout::has_features<ENV>::value ? 0.f : out.x[ENV::FUT_SRC]);
}

// mpg_model_step: one lane per row, od entries per observation row
template <class ENV>
__global__ void __launch_bounds__(64) k_model_step(int rows, int od_arg, const float* __restrict__ obs, const float* __restrict__ act,
                                                   const float* __restrict__ eps, float* __restrict__ obs_next, float* __restrict__ rew_out) {
    constexpr int OD = fixed_width<ENV, XW>();
    const int od = OD ? OD : od_arg;
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (size_t)rows) return;
    float x[reads<ENV>()], xn[XW], a[2] = {0.f, 0.f}, rew;
#pragma unroll
    for (int k = 0; k < reads<ENV>(); ++k) x[k] = obs[i * od + k];
#pragma unroll
    for (int k = 0; k < ENV::ACT; ++k) a[k] = act[i * ENV::ACT + k];
    model_row<ENV>(x, a, eps ? eps[i] : 0.f, xn, rew);
#pragma unroll
    for (int k = 0; k < XW; ++k)
        if (k < od) obs_next[i * od + k] = xn[k];
    rew_out[i] = rew;
}

// a rollout launch's policy arguments (A of policy_pass.h); OD: fixed_width of the instantiation
template <int OD>
struct PolicyArgs {
    const float* params;       // policy network, Keras order
    const float* pack;         // nullable: packed forward image of W2 (weight cache)
    int* status;               // nullable: MPG_STATUS_* word of the caller
    int out_tanh;
    float out_scale;
    int obs_dim;               // the network's input width = the row stride of the observations
    float scale[XW];           // obs_scale (1 beyond obs_dim)
};
template <int OD>
__device__ __forceinline__ int obs_dim_of(const PolicyArgs<OD>& a) { return OD ? OD : a.obs_dim; }

// One evaluation on the group's observations sObs [16][od] (policy_pass::stage): k_forward<IN, OU, PK, 1> for unit g as
// mpg_policy_action launches it without noise - the action under the cfg's output rule, its NaN test - to sAct [16][OU] (0 beyond
// `rows`), written by wave 0's own lanes: lane tid < 16 OU forms output tid % OU of row tid / OU.
template <int IN, int OU, class A>
__device__ __forceinline__ void pass(const A& a, int rows, long g, const float* sObs, float* smem, float* sAct, const Lane& L,
                                     const float (&w2)[128], const SmallRegs<IN, OU>& r, float b3v, float& zmax, bool& saw_nan) {
    const float pz = policy_pass::stage<IN, OU>(a, rows, g, sObs, smem, L, w2, r, zmax, saw_nan);
    const int tid = threadIdx.x;
    if (tid < GROUP * OU) {
        const int row = tid / OU, o = tid % OU;
        float y = 0.f;
        if (g * GROUP + row < rows) {
            float z = out_preact<out_stride<OU>()>(policy_pass::part_of<IN>(smem), b3v, row, o);
            y = a.out_tanh ? a.out_scale * tanhf(z) : z;
            y += pz;
            saw_nan |= y != y;
        }
        sAct[tid] = y;
    }
}

constexpr int EPS_STEPS = NTHREAD / GROUP;      // steps of model noise the group keeps in LDS: one value per thread and refill

// The policy's closed loop on the model in ONE launch: for t < steps the pair mpg_policy_action (sigma 0) + mpg_model_step, 2 * steps
// launches of at most one wave per CU each, every policy launch fetching the weights again.  The resident plan of policy_pass.h: one
// workgroup owns 16 trajectories for all steps and loads the policy's registers once, lane i < 16 of wave 0 holds in registers what the
// model reads of trajectory i's row (reads<ENV>() entries; the rest of a row - look-ahead entries, the double pendulum's last three - only
// passes through sObs), per step the rows go to the pass through sObs and the actions come back through sAct.  Per step t the row BEFORE the step goes to
// obs_traj[(t n + i) od ..], the action as the pass formed it to act_traj[(t n + i) ACT ..], the raw reward to rew_traj[t n + i]
// (mpg_eval_rollout's record); the row behind the last step to last_obs.  Nothing the kernel wrote is read back.  The model noise is
// the one input that is not read in the prologue alone - 1024 steps of it do not fit LDS beside the pass: every EPS_STEPS steps the
// whole workgroup fetches the next EPS_STEPS x 16 values, one per thread, into sEps in front of the step's first barrier.  Wave 0 takes
// its step's value out of sEps right behind that barrier: the other waves reach the next refill only through the pass's barriers, which
// wave 0 enters after that read.
template <class ENV, bool PK, int IN>
__global__ void __launch_bounds__(NTHREAD, 2) k_model_rollout(const PolicyArgs<fixed_width<ENV, IN>()> pa, int n, int steps,
                                                              const float* __restrict__ obs0, const float* __restrict__ eps,
                                                              float* __restrict__ obs_traj, float* __restrict__ act_traj,
                                                              float* __restrict__ rew_traj, float* __restrict__ last_obs) {
    constexpr int OU = ENV::ACT;
    __shared__ __attribute__((aligned(16))) float smem[policy_pass::smem_floats<IN, OU>()];
    __shared__ __attribute__((aligned(16))) float sObs[GROUP * XW];
    __shared__ float sAct[GROUP * 2];
    __shared__ float sEps[EPS_STEPS * GROUP];
    const int od = obs_dim_of(pa);
    const Lane L;
    float w2[128];
    SmallRegs<IN, OU> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, IN, OU>(pa, 2 * OU, L, w2, r, b3v);
    const int tid = threadIdx.x, i = blockIdx.x * GROUP + tid;
    const bool traj = tid < GROUP && i < n;
    constexpr int NR = reads<ENV>();
    float x[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) x[k] = 0.f;
    if (traj) {
        const float* const src = obs0 + (size_t)i * od;
#pragma unroll
        for (int k = 0; k < XW; ++k)
            if (k < od) {
                const float v = src[k];
                if (k < NR) x[k < NR ? k : 0] = v;
                sObs[tid * od + k] = v;
            }
    }
    for (int t = 0; t < steps; ++t) {
        if (t % EPS_STEPS == 0) {
            const int ts = t + tid / GROUP, tr = blockIdx.x * GROUP + tid % GROUP;
            float z = 0.f;
            if (eps && ts < steps && tr < n) z = eps[(size_t)ts * n + tr];
            sEps[tid] = z;
        }
        lds_barrier();                                   // sObs of this step is complete (and the previous pass's LDS is free)
        float e = 0.f;
        if (tid < GROUP) e = sEps[(t % EPS_STEPS) * GROUP + tid];
        pass<IN, OU>(pa, n, blockIdx.x, sObs, smem, sAct, L, w2, r, b3v, zmax, saw_nan);
        if (tid >= 64) continue;                         // wave 0 wrote sAct itself: LDS is in order within a wave
        __builtin_amdgcn_wave_barrier();
        if (traj) {
            float a[2] = {0.f, 0.f}, xn[XW], rew;
#pragma unroll
            for (int k = 0; k < OU; ++k) a[k] = sAct[tid * OU + k];
            const size_t row = (size_t)t * (size_t)n + (size_t)i;
            {   // the row before the step, as the pass read it: the lane's own entries, the others out of sObs
                float* const ot = obs_traj + row * od;
#pragma unroll
                for (int k = 0; k < XW; ++k)
                    if (k < od) ot[k] = k < NR ? x[k < NR ? k : 0] : sObs[tid * od + k];
            }
#pragma unroll
            for (int k = 0; k < OU; ++k) act_traj[row * OU + k] = a[k];
            model_row<ENV>(x, a, e, xn, rew);
            rew_traj[row] = rew;
            if (t == steps - 1) {
                float* const lo = last_obs + (size_t)i * od;
#pragma unroll
                for (int k = 0; k < XW; ++k)
                    if (k < od) lo[k] = xn[k];
            } else {
#pragma unroll
                for (int k = 0; k < XW; ++k)
                    if (k < od) sObs[tid * od + k] = xn[k];
            }
#pragma unroll
            for (int k = 0; k < NR; ++k) x[k] = xn[k];
        }
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// launch(ENV{}, std::integral_constant<int, IN>{}) for the cfg's model and width
template <class Launch>
void with_model(const mpg_cfg_t* cfg, Launch&& launch) {
    if (cfg->env_kind == MPG_ENV_INVERTED_DOUBLE_PENDULUM) launch(rollout::DoublePendulum{}, std::integral_constant<int, 16>{});
    else if (cfg->env_kind == MPG_ENV_INVERTED_PENDULUM) launch(rollout::Pendulum{}, std::integral_constant<int, 4>{});
    else if (cfg->obs_dim > 6) launch(rollout::PathTracking{}, std::integral_constant<int, 16>{});
    else launch(rollout::PathTracking{}, std::integral_constant<int, 6>{});
}

}  // namespace model_rollout

extern "C" int mpg_model_step(const mpg_cfg_t* cfg, int rows, const float* obs, const float* act, const float* eps, float* obs_next,
                              float* rew, mpg_stream_t stream) {
    using namespace model_rollout;
    if (int rc = model_cfg_refusal("mpg_model_step", cfg)) return rc;
    MPG_REQUIRE(rows > 0, "mpg_model_step: no rows (rows %d)", rows);
    MPG_REQUIRE(obs && act && obs_next && rew, "mpg_model_step: null pointer");
    if (int rc = tanh_range_refusal("mpg_model_step", cfg)) return rc;
    hipStream_t s = mpg_stream(stream);
    with_model(cfg, [&](auto env, auto) {
        hipLaunchKernelGGL(k_model_step<decltype(env)>, dim3((rows + 63) / 64), dim3(64), 0, s, rows, cfg->obs_dim, obs, act, eps, obs_next,
                           rew);
    });
    MPG_CHECK_LAUNCH("mpg_model_step");
    return MPG_OK;
}

extern "C" int mpg_model_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int steps, const float* obs0, const float* eps,
                                 float* obs_traj, float* act_traj, float* rew_traj, float* last_obs, mpg_stream_t stream) {
    using namespace model_rollout;
    if (int rc = model_cfg_refusal("mpg_model_rollout", cfg)) return rc;
    MPG_REQUIRE(n > 0, "mpg_model_rollout: no trajectories (n %d)", n);
    MPG_REQUIRE(steps >= 1, "mpg_model_rollout: steps >= 1 (got %d)", steps);
    // (what bounds one launch's run time, as mpg_eval_rollout's bound does)
    MPG_REQUIRE(steps <= 1024, "mpg_model_rollout: steps <= 1024 (got %d)", steps);
    MPG_REQUIRE(policy_params && obs0 && obs_traj && act_traj && rew_traj && last_obs, "mpg_model_rollout: null pointer");
    if (int rc = tanh_range_refusal("mpg_model_rollout", cfg)) return rc;
    const int blocks = (n + GROUP - 1) / GROUP;
    hipStream_t s = mpg_stream(stream);
    with_model(cfg, [&](auto env, auto in) {
        typedef decltype(env) ENV;
        constexpr int IN = decltype(in)::value;
        PolicyArgs<fixed_width<ENV, IN>()> pa;
        pa.params = policy_params;
        pa.pack = weight_cache_lookup(cfg, make_net(policy_params, cfg->obs_dim, 2 * cfg->act_dim).W2, 0);
        pa.status = mpg_status_of(cfg);
        const OutSpec po = policy_out(cfg);              // as mpg_policy_action forms it
        pa.out_tanh = po.out_tanh; pa.out_scale = po.out_scale;
        pa.obs_dim = cfg->obs_dim;
        for (int i = 0; i < XW; ++i) pa.scale[i] = i < cfg->obs_dim ? cfg->obs_scale[i] : 1.f;
        if (pa.pack)
            hipLaunchKernelGGL((k_model_rollout<ENV, true, IN>), dim3(blocks), dim3(NTHREAD), 0, s, pa, n, steps, obs0, eps, obs_traj,
                               act_traj, rew_traj, last_obs);
        else
            hipLaunchKernelGGL((k_model_rollout<ENV, false, IN>), dim3(blocks), dim3(NTHREAD), 0, s, pa, n, steps, obs0, eps, obs_traj,
                               act_traj, rew_traj, last_obs);
    });
    MPG_CHECK_LAUNCH("mpg_model_rollout");
    return MPG_OK;
}
