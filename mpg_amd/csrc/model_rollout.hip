// The differentiable models on their own: mpg_model_step, one rollout_out of the model a cfg names (k_model_step, one lane per row),
// and mpg_model_rollout, a policy's closed loop on that model in one launch (k_model_rollout) - what mpg_eval_rollout is for the real
// envs, for the models the learners optimise through (rollout_common.h: PathTracking, Pendulum, DoublePendulum), the double pendulum
// included, whose real env does not exist here.  Also here, for that model alone: the model as an ENVIRONMENT (namespace model_env below:
// mpg_model_env_reset / _step / _step_store_reset and mpg_worker_rollout_model, a worker sample on it in one launch), on the same row
// step.
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

// ---- The double pendulum's model as an ENVIRONMENT (mpg_model_env_*, mpg_worker_rollout_model; include/mpg_hip.h, DESIGN.md section 7
// f20): the step is model_row_call<DoublePendulum> - the body k_model_step and k_model_rollout call -, a done law on the model's tip
// height, an episode limit on a per-agent step count (`age`), and a reset law of the shape of gym's reset_model.  The env keeps no
// state beside the observation row and the age.  The done test and the reset draw are bodies of their own that are NOT inlined, for
// model_row_call's reason: the three kernels that step and the two that re-draw call the same instructions, so the chain of launches
// and the one launch agree in bits.
namespace model_env {
using DP = rollout::DoublePendulum;
constexpr int OD = DP::NFEAT;                  // 11
constexpr int NR = reads<DP>();                // the 8 entries the model reads; entries 8 .. 10 of every row the env forms are zero
constexpr uint32_t RESET_TAG = 0x64706d65u;    // Philox counter word 3 of the reset draw (and RESET_TAG + 1)

// gym's done = (y <= 1) on the MODEL's tip height y = 0.6 cos t1 + 0.6 cos t2 (upright: 1.2), from entries 3 and 4 of the new row: two
// rounded products and one rounded sum, no contraction - what __fmul_rn / __fadd_rn say, written as plain operators under a contraction
// rule of the function's own: the two intrinsics are inline functions of a header compiled under the default rule, the compiler fused
// their product and sum here (v_mul, v_fmac), and a rule set around the CALLS does not reach into them.  The comparison is negated: a
// NaN row is done, and is re-drawn.
__device__ __noinline__ int fell(float cos1, float cos2) {
#pragma clang fp contract(off)
    const float y1 = 0.6f * cos1, y2 = 0.6f * cos2;
    const float tip_y = y1 + y2;
    return !(tip_y > 1.0f) ? 1 : 0;
}
// done = fell | truncated; truncated: the step that makes the agent's count max_steps (0: no limit)
__device__ __forceinline__ int done_of(const float (&xn)[XW], int age, int max_steps) {
    return fell(xn[3], xn[4]) | ((max_steps > 0 && age + 1 >= max_steps) ? 1 : 0);
}

// The reset law for agent i on the Philox stream (key, counter (c1, c2), i): p, theta1, theta2 ~ U(-0.1, 0.1) from the first block's
// words 0 .. 2, pdot, theta1dot, theta2dot ~ 0.1 N(0, 1) by Box-Muller from the second block's two word pairs (the fourth deviate is
// not used) - the uniform and Box-Muller idioms of the real envs' reset laws.  Returns the 8 leading features of that state.
struct ResetRow {
    float x[8];
};
__device__ __noinline__ ResetRow reset_row(uint32_t i, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2) {
    const Philox4 a = philox4x32_10(i, c1, c2, RESET_TAG, k0, k1);
    const Philox4 b = philox4x32_10(i, c1, c2, RESET_TAG + 1u, k0, k1);
    const float p = 0.2f * u01(a.v[0]) - 0.1f, t1 = 0.2f * u01(a.v[1]) - 0.1f, t2 = 0.2f * u01(a.v[2]) - 0.1f;
    const float r0 = sqrtf(-2.f * logf(u01(b.v[0]))), r1 = sqrtf(-2.f * logf(u01(b.v[2])));
    float s0, c0, s1, cc1;
    sincosf(6.283185307179586f * u01(b.v[1]), &s0, &c0);
    sincosf(6.283185307179586f * u01(b.v[3]), &s1, &cc1);
    (void)s1;
    ResetRow r;
    r.x[0] = p;
    sincosf(t1, &r.x[1], &r.x[3]);
    sincosf(t2, &r.x[2], &r.x[4]);
    r.x[5] = 0.1f * (r0 * c0);
    r.x[6] = 0.1f * (r0 * s0);
    r.x[7] = 0.1f * (r1 * cc1);
    return r;
}
__device__ __forceinline__ void load_row(const float* __restrict__ src, float (&x)[NR]) {
#pragma unroll
    for (int k = 0; k < NR; ++k) x[k] = src[k];
}
// a row the env formed: the 8 entries and three zeros
__device__ __forceinline__ void store_row(float* __restrict__ dst, const float (&x)[NR]) {
#pragma unroll
    for (int k = 0; k < OD; ++k) dst[k] = k < NR ? x[k < NR ? k : 0] : 0.f;
}

// mpg_model_env_reset: one lane per agent; an agent whose mask byte is 0 is not touched
__global__ void __launch_bounds__(64) k_model_env_reset(int n, float* __restrict__ obs_io, int* __restrict__ age_io,
                                                        const uint8_t* __restrict__ mask, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n || (mask != nullptr && !mask[i])) return;
    const ResetRow r = reset_row((uint32_t)i, k0, k1, c1, c2);
    store_row(obs_io + (size_t)i * OD, r.x);
    age_io[i] = 0;
}

// mpg_model_env_step: k_model_step's row step, the done law and the agent's count
__global__ void __launch_bounds__(64) k_model_env_step(int n, const float* __restrict__ obs, const float* __restrict__ act, int max_steps,
                                                       int* __restrict__ age_io, float* __restrict__ obs_next, float* __restrict__ rew_out,
                                                       uint8_t* __restrict__ done) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float x[NR], xn[XW], a[2] = {0.f, 0.f}, rew;
    load_row(obs + (size_t)i * OD, x);
    a[0] = act[i];
    const int age = age_io[i];
    model_row<DP>(x, a, 0.f, xn, rew);
    float* const on = obs_next + (size_t)i * OD;
#pragma unroll
    for (int k = 0; k < OD; ++k) on[k] = xn[k];
    rew_out[i] = rew;
    done[i] = (uint8_t)done_of(xn, age, max_steps);
    age_io[i] = age + 1;
}

// mpg_model_env_step_store_reset: the step, the transition to ring slot (next_idx + i) % capacity - the row BEFORE the step as it
// stands in obs_io, all 11 entries -, and the re-draw of a done agent, in the order of the three calls it replaces
__global__ void __launch_bounds__(64) k_model_env_step_store_reset(int n, float* __restrict__ obs_io, const float* __restrict__ act,
                                                                   int max_steps, int* __restrict__ age_io, RingPtrs ring, int capacity,
                                                                   int next_idx, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2,
                                                                   uint8_t* __restrict__ done_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float* const row = obs_io + (size_t)i * OD;
    float x[NR], tail[OD - NR], xn[XW], a[2] = {0.f, 0.f}, rew;
    load_row(row, x);
#pragma unroll
    for (int k = NR; k < OD; ++k) tail[k - NR] = row[k];
    a[0] = act[i];
    const int age = age_io[i];
    const size_t slot = (size_t)(((long)next_idx + i) % capacity);
    float* const ro = ring.obs + slot * OD;
#pragma unroll
    for (int k = 0; k < OD; ++k) ro[k] = k < NR ? x[k < NR ? k : 0] : tail[k < NR ? 0 : k - NR];
    ring.act[slot] = a[0];
    model_row<DP>(x, a, 0.f, xn, rew);
    float* const ro2 = ring.obs2 + slot * OD;
#pragma unroll
    for (int k = 0; k < OD; ++k) ro2[k] = xn[k];
    ring.rew[slot] = rew;
    const int dn = done_of(xn, age, max_steps);
    ring.done[slot] = (uint8_t)dn;
    if (done_out) done_out[i] = (uint8_t)dn;
#pragma unroll
    for (int k = 0; k < NR; ++k) x[k] = xn[k];
    if (dn) {
        const ResetRow r = reset_row((uint32_t)i, k0, k1, c1, c2);
#pragma unroll
        for (int k = 0; k < NR; ++k) x[k] = r.x[k];
    }
    store_row(row, x);
    age_io[i] = dn ? 0 : age + 1;
}

// What wave 0 needs of a worker rollout's arguments once per iteration.  They rest in LDS and are read where they are used, as
// CpRolloutEnvArgs does (env_cart_pole.hip) and for its reason: the kernel has no register to spare (k_model_rollout's budget).
struct RolloutArgs {
    RingPtrs ring;
    float *obs_io, *act_out;
    int* age_io;
    uint8_t* done_out;
    uint32_t k0, k1, nk0, nk1;     // env key, exploration-noise key
    uint64_t env_ctr, noise_ctr;   // the counters of iteration 0, carried as 64-bit sums
    uint32_t capacity;
    int max_steps;
    float sigma;
};

// The exploration noise of mpg_policy_action (k_forward) on row gr's one output, from its Philox draw at the 64-bit counter (c1, c2),
// then its NaN test (pass() tested the action before the noise: a NaN there is a NaN here)
__device__ __forceinline__ float explore(float y, float sigma, long gr, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2, bool& saw_nan) {
    if (sigma > 0.f) {   // OffPolicyWorker.sample: action += N(0, sigma), worker.py:97-98
        const Philox4 p = philox4x32_10((uint32_t)gr, c1, c2, 0x5eedu, k0, k1);
        const float u1 = u01(p.v[0]), u2 = u01(p.v[1]);
        y = add_gauss_noise(y, sigma, u1, u2);
    }
    saw_nan |= y != y;
    return y;
}

// OffPolicyWorker.sample's `iters` iterations (worker.py:91-119: policy -> + N(0, sigma) -> env.step -> ring -> env.reset) on the model
// env in ONE launch: `iters` consecutive pairs of mpg_policy_action (k_forward<16, 1, PK, 1>) and k_model_env_step_store_reset, with the
// noise and env counters and the ring position advancing by one / one / n per pair.  k_model_rollout's resident plan: one workgroup
// owns 16 agents for all iterations and loads the policy's registers once; lane i < 16 of wave 0 holds the 8 entries the model reads
// of agent i's row and its age in registers; per iteration the rows go to the pass through sObs and the actions come back through
// sAct.  Per iteration `it` the lane does what k_model_env_step_store_reset does, in its order: ring row (obs, act) at slot (next_idx +
// it * n + i) % capacity, the row step, (obs2, rew, done), the re-draw keyed (env key, env counter + it) if done, and the next row - into
// sObs instead of obs_io.  Entries 8 .. 10 of a row are whatever obs_io held in iteration 0 and zeros from then on (every row the env
// forms ends in zeros): the ring row takes them out of sObs.  obs_io, age_io, act_out and done_out are written after the LAST iteration
// only (what the chain leaves behind).  Every loop is bounded by `iters`; no workgroup waits for another; global memory is read in the
// prologue only and nothing the kernel wrote is read back.  The host refuses iters * n > capacity: two iterations would write one ring
// slot from different workgroups.
template <bool PK>
__global__ void __launch_bounds__(NTHREAD, 2) k_worker_rollout_model(const PolicyArgs<OD> pa, int n, int iters, RolloutArgs ra,
                                                                     int next_idx) {
    constexpr int IN = 16, OU = 1;
    __shared__ __attribute__((aligned(16))) float smem[policy_pass::smem_floats<IN, OU>()];
    __shared__ __attribute__((aligned(16))) float sObs[GROUP * XW];
    __shared__ float sAct[GROUP * 2];
    __shared__ RolloutArgs sArg;
    const Lane L;
    float w2[128];
    SmallRegs<IN, OU> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, IN, OU>(pa, 2 * OU, L, w2, r, b3v);
    const int tid = threadIdx.x, i = blockIdx.x * GROUP + tid;
    const bool env_lane = tid < GROUP && i < n;
    float x[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) x[k] = 0.f;
    int age = 0;
    if (env_lane) {
        const float* const src = ra.obs_io + (size_t)i * OD;
#pragma unroll
        for (int k = 0; k < OD; ++k) {
            const float v = src[k];
            if (k < NR) x[k < NR ? k : 0] = v;
            sObs[tid * OD + k] = v;
        }
        age = ra.age_io[i];
    }
    if (tid == 0) sArg = ra;
    // the agent's ring slot: (next_idx + it * n + i) % capacity
    uint32_t slot = env_lane ? (uint32_t)(((long)next_idx + i) % (long)ra.capacity) : 0u;
    for (int it = 0; it < iters; ++it) {
        lds_barrier();                                   // sObs of this iteration is complete (and the previous pass's LDS is free)
        pass<IN, OU>(pa, n, blockIdx.x, sObs, smem, sAct, L, w2, r, b3v, zmax, saw_nan);
        if (tid >= 64) continue;                         // wave 0 wrote sAct itself: LDS is in order within a wave
        __builtin_amdgcn_wave_barrier();
        if (!env_lane) continue;
        const uint64_t nc = sArg.noise_ctr + (uint64_t)it;
        float a[2] = {0.f, 0.f}, xn[XW], rew;
        a[0] = explore(sAct[tid], sArg.sigma, i, sArg.nk0, sArg.nk1, (uint32_t)nc, (uint32_t)(nc >> 32), saw_nan);
        {   // the row before the step, as the pass read it: the lane's own entries, the last three out of sObs
            float* const ro = sArg.ring.obs + (size_t)slot * OD;
#pragma unroll
            for (int k = 0; k < OD; ++k) ro[k] = k < NR ? x[k < NR ? k : 0] : sObs[tid * OD + k];
        }
        sArg.ring.act[slot] = a[0];
        model_row<DP>(x, a, 0.f, xn, rew);
        {
            float* const ro2 = sArg.ring.obs2 + (size_t)slot * OD;
#pragma unroll
            for (int k = 0; k < OD; ++k) ro2[k] = xn[k];
        }
        sArg.ring.rew[slot] = rew;
        const int dn = done_of(xn, age, sArg.max_steps);
        sArg.ring.done[slot] = (uint8_t)dn;
#pragma unroll
        for (int k = 0; k < NR; ++k) x[k] = xn[k];
        age = age + 1;
        if (dn) {
            const uint64_t ec = sArg.env_ctr + (uint64_t)it;
            const ResetRow rr = reset_row((uint32_t)i, sArg.k0, sArg.k1, (uint32_t)ec, (uint32_t)(ec >> 32));
#pragma unroll
            for (int k = 0; k < NR; ++k) x[k] = rr.x[k];
            age = 0;
        }
        if (it == iters - 1) {
            sArg.act_out[i] = a[0];
            uint8_t* const dp = sArg.done_out;
            if (dp) dp[i] = (uint8_t)dn;
            store_row(sArg.obs_io + (size_t)i * OD, x);
            sArg.age_io[i] = age;
        } else {
            store_row(sObs + tid * OD, x);
        }
        slot += (uint32_t)n;
        if (slot >= sArg.capacity) slot -= sArg.capacity;
    }
    policy_pass::report(pa, zmax, saw_nan);
}
}  // namespace model_env

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

// the model env's reset law (gym's reset_model: U(-0.1, 0.1) positions, 0.1 N(0, 1) velocities) for the agents the mask names
extern "C" int mpg_model_env_reset(const mpg_cfg_t* cfg, int n, float* obs_io, int* age_io, const uint8_t* done_mask, uint64_t seed,
                                   uint64_t ctr, mpg_stream_t stream) {
    using namespace model_rollout;
    using namespace model_rollout::model_env;
    if (int rc = model_env_cfg_refusal("mpg_model_env_reset", cfg)) return rc;
    MPG_REQUIRE(obs_io && age_io, "mpg_model_env_reset: null pointer");
    if (int rc = model_env_size_refusal("mpg_model_env_reset", n, 0, nullptr, 0, 0)) return rc;
    hipLaunchKernelGGL(k_model_env_reset, dim3((n + 63) / 64), dim3(64), 0, mpg_stream(stream), n, obs_io, age_io, done_mask,
                       MPG_KEY_CTR(seed, ctr));
    MPG_CHECK_LAUNCH("mpg_model_env_reset");
    return MPG_OK;
}

// one env step: mpg_model_step's obs_next and raw rew, done = fell | truncated, age + 1
extern "C" int mpg_model_env_step(const mpg_cfg_t* cfg, int n, const float* obs, const float* act, int max_steps, int* age_io,
                                  float* obs_next, float* rew, uint8_t* done, mpg_stream_t stream) {
    using namespace model_rollout;
    using namespace model_rollout::model_env;
    if (int rc = model_env_cfg_refusal("mpg_model_env_step", cfg)) return rc;
    MPG_REQUIRE(obs && act && age_io && obs_next && rew && done, "mpg_model_env_step: null pointer");
    if (int rc = model_env_size_refusal("mpg_model_env_step", n, max_steps, nullptr, 0, 0)) return rc;
    hipLaunchKernelGGL(k_model_env_step, dim3((n + 63) / 64), dim3(64), 0, mpg_stream(stream), n, obs, act, max_steps, age_io, obs_next, rew,
                       done);
    MPG_CHECK_LAUNCH("mpg_model_env_step");
    return MPG_OK;
}

// mpg_model_env_step + mpg_replay_add + mpg_model_env_reset(mask = done) as one launch (k_model_env_step_store_reset: bit-identical
// obs_io, age_io, ring arrays and done flags)
extern "C" int mpg_model_env_step_store_reset(const mpg_cfg_t* cfg, int n, float* obs_io, const float* act, int max_steps, int* age_io,
                                              int capacity, int next_idx, float* ring_obs, float* ring_act, float* ring_rew,
                                              float* ring_obs2, uint8_t* ring_done, uint64_t seed, uint64_t ctr, uint8_t* done_out,
                                              mpg_stream_t stream) {
    using namespace model_rollout;
    using namespace model_rollout::model_env;
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    if (int rc = model_env_cfg_refusal("mpg_model_env_step_store_reset", cfg)) return rc;
    MPG_REQUIRE(obs_io && act && age_io && ring.obs && ring.act && ring.rew && ring.obs2 && ring.done,
                "mpg_model_env_step_store_reset: null pointer");
    if (int rc = model_env_size_refusal("mpg_model_env_step_store_reset", n, max_steps, &ring, capacity, next_idx)) return rc;
    hipLaunchKernelGGL(k_model_env_step_store_reset, dim3((n + 63) / 64), dim3(64), 0, mpg_stream(stream), n, obs_io, act, max_steps, age_io,
                       ring, capacity, next_idx, MPG_KEY_CTR(seed, ctr), done_out);
    MPG_CHECK_LAUNCH("mpg_model_env_step_store_reset");
    return MPG_OK;
}

// worker.py:91-119 on the model env: `iters` consecutive pairs mpg_policy_action + mpg_model_env_step_store_reset (noise_ctr + it, ring
// position (next_idx + it * n) % capacity, env_ctr + it) as one launch (k_worker_rollout_model: bit-identical observations, ages,
// actions, done flags, ring arrays and status word)
extern "C" int mpg_worker_rollout_model(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* obs_io, int* age_io,
                                        int max_steps, float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr, float* act_out,
                                        int capacity, int next_idx, float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2,
                                        uint8_t* ring_done, uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out, mpg_stream_t stream) {
    using namespace model_rollout;
    using namespace model_rollout::model_env;
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    if (int rc = model_env_cfg_refusal("mpg_worker_rollout_model", cfg)) return rc;
    MPG_REQUIRE(policy_params && obs_io && age_io && act_out && ring.obs && ring.act && ring.rew && ring.obs2 && ring.done,
                "mpg_worker_rollout_model: null pointer");
    if (int rc = model_env_size_refusal("mpg_worker_rollout_model", n, max_steps, &ring, capacity, next_idx)) return rc;
    MPG_REQUIRE(iters >= 1, "mpg_worker_rollout_model: iters >= 1 (got %d)", iters);
    // (what bounds one launch's run time, as the worker rollouts on the real envs bound theirs)
    MPG_REQUIRE(iters <= 1024, "mpg_worker_rollout_model: iters <= 1024 (got %d)", iters);
    // two iterations would write one slot from different workgroups with no order between them
    MPG_REQUIRE((long)iters * n <= capacity, "mpg_worker_rollout_model: iters * n = %ld transitions do not fit the ring's capacity %d",
                (long)iters * n, capacity);
    PolicyArgs<OD> pa;
    pa.params = policy_params;
    pa.pack = weight_cache_lookup(cfg, make_net(policy_params, OD, 2).W2, 0);
    pa.status = mpg_status_of(cfg);
    const OutSpec po = policy_out(cfg);              // as mpg_policy_action forms it
    pa.out_tanh = po.out_tanh; pa.out_scale = po.out_scale;
    pa.obs_dim = OD;
    for (int i = 0; i < XW; ++i) pa.scale[i] = i < OD ? cfg->obs_scale[i] : 1.f;
    RolloutArgs ra;
    ra.ring = ring;
    ra.obs_io = obs_io; ra.act_out = act_out; ra.age_io = age_io; ra.done_out = done_out;
    ra.k0 = (uint32_t)env_seed; ra.k1 = (uint32_t)(env_seed >> 32);
    ra.nk0 = (uint32_t)noise_seed; ra.nk1 = (uint32_t)(noise_seed >> 32);
    ra.env_ctr = env_ctr; ra.noise_ctr = noise_ctr;
    ra.capacity = (uint32_t)capacity; ra.max_steps = max_steps; ra.sigma = explore_sigma;
    const int blocks = (n + GROUP - 1) / GROUP;
    hipStream_t s = mpg_stream(stream);
    mpg_prof_begin(mpg_prof_of(cfg), 2, s);
    if (pa.pack)
        hipLaunchKernelGGL(k_worker_rollout_model<true>, dim3(blocks), dim3(NTHREAD), 0, s, pa, n, iters, ra, next_idx);
    else
        hipLaunchKernelGGL(k_worker_rollout_model<false>, dim3(blocks), dim3(NTHREAD), 0, s, pa, n, iters, ra, next_idx);
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_rollout_model");
    return MPG_OK;
}
