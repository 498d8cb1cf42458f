// InvertedPendulumConti-v0 as an analytic kernel: the reference steps this environment with MuJoCo
// (envs_and_models/inverted_pendulum_conti.py:5-30 on inverted_pendulum_conti.xml); here the same model - cart on a
// slider, one pole on a hinge, capsule geometry at the default density 1000 kg/m^3, joint damping 1, motor gear 100 with
// ctrlrange +-3, gravity 9.81, integrator RK4, timestep 0.02, frame_skip 2 - is written as the closed-form cart-pole
// equations and integrated with the classical Runge-Kutta scheme, one lane per agent, state in registers.
//
//   (M + m) pdd + m l cos(th) thdd = F - b_x pd + m l sin(th) thd^2
//   m l cos(th) pdd + (I + m l^2) thdd = m g l sin(th) - b_th thd            th measured from the pole's rest axis + th0
//
// PARITY UNPINNED: MuJoCo is not installable here, so no reference run can pin these numbers; the kernel is checked
// against oracle/mpg_oracle.py:InvertedPendulumContiOracle (the float64 statement of the same formulas), and DESIGN.md
// says so.  obs = [p, theta, pdot, thetadot] (:27-28); reward (:12-16); done = not(|p| < 2 and |theta| <= 0.2) (:17-18);
// reset: U(-0.01, 0.01) on all four (:21-25) from Philox(seed, ctr, agent).
//
// State block: rows 0..3 of the opaque [MPG_ENV_STATE_DIM][n] array (rows 4..7 unused).
//
// Also here, beside the device functions it steps the agents with: mpg_worker_rollout_pendulum, a worker sample's iterations on this
// env in one launch (k_worker_rollout_pendulum), mpg_worker_sample_rollout_pendulum, the same for the tanh-squashed Gaussian policy
// (k_worker_sample_rollout_pendulum), mpg_env_rollout_pendulum, the learner's n real-env steps from a replay batch in one launch
// (k_env_rollout_pendulum), and mpg_eval_rollout_pendulum, an evaluation's steps with their trajectory in one launch
// (k_eval_rollout_pendulum).
#include <type_traits>

#include "env_internal.h"

// The worker's policy pass rides in the one-launch worker sample (k_worker_rollout_pendulum, below).  The network engine is compiled
// here as every other translation unit compiles it - contraction allowed - although this file is built with -ffp-contract=off for the
// cart-pole's arithmetic (the step and the fused kernels must round identically): the pragma is lexical, the environment code below is
// back under "off".
#pragma clang fp contract(fast)
#include "mlp_core.h"
#include "gauss_head.h"
#include "policy_pass.h"

// The pieces of policy_pass.h for the pendulum's policy: four inputs and the network's two outputs (mean | log-std).  OU = 1, the
// deterministic worker: ONE used output; the used output of row `row` is formed by lane `row` of wave 0, the lane that holds the row's
// agent (S4, one lane per agent), so the action goes from the pass to the noise to the env step in a register.  OU = 2, the
// tanh-squashed Gaussian policy: BOTH outputs as policy_logits launches them for mpg_policy_sample_squashed - k_forward<4, 2, PK, 1>: no
// action range on the logits, and the linear output only (gauss::squash_refusal leaves no other) - then the row's element of the
// standard-normal stream and gauss::squash_row itself.  The two logits of row `row` are formed by lanes 2 row and 2 row + 1 of wave 0
// and go through sLogit [16][2] to lane `row`: LDS is in order within a wave.
// gauss_head.h is included above, under this block's contraction rule, as learner_api.hip compiles it; of what squash_row calls for the
// ACTION - the double-precision exp of sigma_of and tanhf - the expansion does not depend on the translation unit's own mode (the
// instructions of both were compared under the two modes: DESIGN.md section 7 f11), and the log-density's expf / log1pf are dead here.
namespace cp_policy {
using namespace mlp;
constexpr int IN = 4;

struct Args {                  // OU = 1
    const float* params;       // policy network, Keras order
    const float* pack;         // nullable: packed forward image of W2 (weight cache)
    int* status;               // nullable: MPG_STATUS_* word of the caller
    int out_tanh;
    float out_scale, sigma;
    uint32_t k0, k1, c1, c2;   // exploration-noise key and the counter of iteration 0
    float scale[IN];           // obs_scale
};
struct SampleArgs {            // OU = 2
    const float* params;
    const float* pack;
    int* status;
    float range, log_r;        // the action range and its logarithm (gauss::log_range)
    uint32_t k0, k1, c1, c2;   // the draw's key and the counter of iteration 0
    float scale[IN];
};
template <int OU> struct args_of { typedef Args type; };
template <> struct args_of<2> { typedef SampleArgs type; };
template <class A>
__device__ __forceinline__ constexpr int obs_dim_of(const A&) { return IN; }

template <int OU>
__host__ __device__ constexpr int smem_floats() { return policy_pass::smem_floats<IN, OU>(); }

// One evaluation on the group's observations sObs [16][4] in LDS (policy_pass::stage): k_forward<4, OU, PK, 1> for unit g.
// OU = 1: as mpg_policy_action launches it, WITHOUT the noise and the NaN test of the action (explore, below); returns row
// threadIdx.x's action on the lanes threadIdx.x < 16 (0 beyond `rows` and on every other lane).
// OU = 2: with the NaN test of the logits, which it leaves in sLogit [16][2] (0 beyond `rows`), written by wave 0's own lanes.
template <int OU>
__device__ __forceinline__ float pass(const typename args_of<OU>::type& a, int rows, long g, const float* sObs, float* smem, float* sLogit,
                                      const Lane& L, const float (&w2)[128], const SmallRegs<IN, OU>& r, float b3v, float& zmax,
                                      bool& saw_nan) {
    static_assert(OU == 1 || OU == 2, "the used output, or both logits");
    constexpr int OS = out_stride<OU>();
    const float pz = policy_pass::stage<IN, OU>(a, rows, g, sObs, smem, L, w2, r, zmax, saw_nan);
    const int tid = threadIdx.x;
    float y = 0.f;
    if constexpr (OU == 1) {
        if (tid < GROUP * OU && g * GROUP + tid < rows) {
            float z = out_preact<OS>(policy_pass::part_of<IN>(smem), b3v, tid, 0);
            y = a.out_tanh ? a.out_scale * tanhf(z) : z;
            y += pz;
        }
    } else if (tid < GROUP * OU) {
        const int row = tid / OU, o = tid % OU;
        if (g * GROUP + row < rows) {
            y = out_preact<OS>(policy_pass::part_of<IN>(smem), b3v, row, o);
            y += pz;
            saw_nan |= y != y;
        }
        sLogit[tid] = y;
        __builtin_amdgcn_wave_barrier();
    }
    return y;
}
// The exploration noise of k_forward on row gr's one output, from its Philox draw at the 64-bit counter (c1, c2), then its NaN test
__device__ __forceinline__ float explore(float y, float sigma, long gr, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2, bool& saw_nan) {
    if (sigma > 0.f) {   // OffPolicyWorker.sample: action += N(0, sigma), worker.py:97-98
        Philox4 p = philox4x32_10((uint32_t)gr, c1, c2, 0x5eedu, k0, k1);
        float u1 = u01(p.v[0]), u2 = u01(p.v[1]);
        y = add_gauss_noise(y, sigma, u1, u2);
    }
    saw_nan |= y != y;
    return y;
}
// Row gr's action from its logits l[2]: element gr of the stream mpg_normal_fill(n, key, counter (c1, c2)) writes - Philox block gr / 4,
// pair (gr / 2) % 2, the even or the odd element of the pair - and k_row_sums<HeadRow<SquashedHead>>'s row body on it.  The log-density is not
// kept: the worker discards it and the ring has no column for it.
__device__ __forceinline__ float sample(const SampleArgs& a, const float* l, int gr, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2) {
    float z_even, z_odd;
    gauss::normal_pair((uint32_t)gr >> 2, (gr >> 1) & 1, k0, k1, c1, c2, z_even, z_odd);
    const float eps = (gr & 1) ? z_odd : z_even;
    float act;
    gauss::squash_row(1, a.range, a.log_r, l, &eps, &act);
    return act;
}
}  // namespace cp_policy
#pragma clang fp contract(off)

namespace {

constexpr double PI_D = 3.14159265358979323846;
constexpr double RHO = 1000.0;
constexpr double capsule_mass(double r, double h) { return RHO * PI_D * r * r * h + RHO * 4.0 / 3.0 * PI_D * r * r * r; }
constexpr double capsule_inertia(double r, double h) {
    return RHO * PI_D * r * r * h * (h * h / 12 + r * r / 4) +
           RHO * 4.0 / 3.0 * PI_D * r * r * r * (2 * r * r / 5 + h * h / 4 + 3 * h * r / 8);
}
// pole: capsule of radius 0.049 from the hinge to (0.001, 0, 0.6)
constexpr double POLE_LEN = 0.60000083333275462;           // hypot(0.001, 0.6)
constexpr float M_CART = (float)capsule_mass(0.1, 0.2);
constexpr float M_POLE = (float)capsule_mass(0.049, POLE_LEN);
constexpr float L_COM = (float)(0.5 * POLE_LEN);
constexpr float I_POLE = (float)capsule_inertia(0.049, POLE_LEN);
constexpr float TH0 = 0.0016666651234593622f;                 // atan2(0.001, 0.6)
constexpr float G = 9.81f, DT = 0.02f, GEAR = 100.f, CTRL = 3.f, DAMP_X = 1.f, DAMP_TH = 1.f;
constexpr int FRAME_SKIP = 2;

struct S4 {
    float p, th, pd, thd;
};

__device__ __forceinline__ S4 deriv(const S4& s, float force) {
    const float th = s.th + TH0;
    float sn, cs;
    sincosf(th, &sn, &cs);
    const float a11 = M_CART + M_POLE, a12 = M_POLE * L_COM * cs, a22 = I_POLE + M_POLE * L_COM * L_COM;
    const float b1 = force - DAMP_X * s.pd + M_POLE * L_COM * sn * s.thd * s.thd;
    const float b2 = M_POLE * G * L_COM * sn - DAMP_TH * s.thd;
    const float idet = 1.f / (a11 * a22 - a12 * a12);
    S4 d;
    d.p = s.pd;
    d.th = s.thd;
    d.pd = (a22 * b1 - a12 * b2) * idet;
    d.thd = (a11 * b2 - a12 * b1) * idet;
    return d;
}
__device__ __forceinline__ S4 axpy(const S4& s, float h, const S4& k) {
    return S4{s.p + h * k.p, s.th + h * k.th, s.pd + h * k.pd, s.thd + h * k.thd};
}

struct StepOut {
    float reward;
    bool done;
};

__device__ __forceinline__ StepOut step_agent(S4& s, float action) {
    // fmaxf(NaN, -3) is -3: a NaN action is handed on, as np.clip / tf.clip_by_value hand it on (a NaN transition with done = 1, not a
    // full push to the left that looks like any other step)
    const float ctrl = fminf(fmaxf(action, -CTRL), CTRL);
    const float force = GEAR * (action != action ? action : ctrl);
#pragma unroll
    for (int f = 0; f < FRAME_SKIP; ++f) {
        const S4 k1 = deriv(s, force);
        const S4 k2 = deriv(axpy(s, 0.5f * DT, k1), force);
        const S4 k3 = deriv(axpy(s, 0.5f * DT, k2), force);
        const S4 k4 = deriv(axpy(s, DT, k3), force);
        const float h6 = DT / 6.f;
        s.p += h6 * (k1.p + 2.f * k2.p + 2.f * k3.p + k4.p);
        s.th += h6 * (k1.th + 2.f * k2.th + 2.f * k3.th + k4.th);
        s.pd += h6 * (k1.pd + 2.f * k2.pd + 2.f * k3.pd + k4.pd);
        s.thd += h6 * (k1.thd + 2.f * k2.thd + 2.f * k3.thd + k4.thd);
    }
    StepOut o;
    o.reward = -(0.01f * s.p * s.p + s.th * s.th) - (0.1f * s.pd * s.pd + 0.1f * s.thd * s.thd);   // :13-15
    o.done = !((fabsf(s.p) < 2.f) && (fabsf(s.th) <= .2f));                                          // :16-17
    return o;
}

__device__ __forceinline__ S4 load(const float* __restrict__ st, size_t N, int i) {
    return S4{st[0 * N + i], st[1 * N + i], st[2 * N + i], st[3 * N + i]};
}
__device__ __forceinline__ void store(float* __restrict__ st, size_t N, int i, const S4& s) {
    st[0 * N + i] = s.p; st[1 * N + i] = s.th; st[2 * N + i] = s.pd; st[3 * N + i] = s.thd;
}
__device__ __forceinline__ void write_obs(float* __restrict__ obs, size_t i, const S4& s) {
    reinterpret_cast<float4*>(obs)[i] = make_float4(s.p, s.th, s.pd, s.thd);
}
__device__ __forceinline__ S4 reset_agent(int i, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2) {
    const Philox4 a = philox4x32_10((uint32_t)i, c1, c2, 0x63617274u, k0, k1);
    return S4{0.02f * u01(a.v[0]) - 0.01f, 0.02f * u01(a.v[1]) - 0.01f, 0.02f * u01(a.v[2]) - 0.01f, 0.02f * u01(a.v[3]) - 0.01f};
}

__global__ void __launch_bounds__(64) k_cp_reset_from_obs(int n, float* __restrict__ st, const float* __restrict__ obs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 o = reinterpret_cast<const float4*>(obs)[i];
    store(st, n, i, S4{o.x, o.y, o.z, o.w});
}

__global__ void __launch_bounds__(64) k_cp_reset(int n, float* __restrict__ st, const uint8_t* __restrict__ mask, uint32_t k0,
                                                 uint32_t k1, uint32_t c1, uint32_t c2, float* __restrict__ obs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    S4 s = load(st, n, i);
    if (mask == nullptr || mask[i]) {
        s = reset_agent(i, k0, k1, c1, c2);
        store(st, n, i, s);
    }
    write_obs(obs, i, s);
}

__global__ void __launch_bounds__(64) k_cp_step(int n, float* __restrict__ st, const float* __restrict__ action,
                                                float* __restrict__ obs, float* __restrict__ reward,
                                                uint8_t* __restrict__ done, uint8_t* __restrict__ done_intended) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    S4 s = load(st, n, i);
    const StepOut o = step_agent(s, action[i]);
    reward[i] = o.reward;
    done[i] = o.done ? 1 : 0;
    if (done_intended) done_intended[i] = o.done ? 1 : 0;
    store(st, n, i, s);
    write_obs(obs, i, s);
}

__global__ void __launch_bounds__(64) k_cp_step_store_reset(int n, float* __restrict__ st, const float* __restrict__ action,
                                                            RingPtrs ring, int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                            uint32_t c1, uint32_t c2, float* __restrict__ obs_out,
                                                            uint8_t* __restrict__ done_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    S4 s = load(st, n, i);
    const float a = action[i];
    const size_t slot = (size_t)((next_idx + i) % capacity);
    write_obs(ring.obs, slot, s);
    ring.act[slot] = a;
    const StepOut o = step_agent(s, a);
    write_obs(ring.obs2, slot, s);
    ring.rew[slot] = o.reward;
    ring.done[slot] = o.done ? 1 : 0;
    if (done_out) done_out[i] = o.done ? 1 : 0;
    if (o.done) s = reset_agent(i, k0, k1, c1, c2);
    store(st, n, i, s);
    write_obs(obs_out, i, s);
}

// ---- the resident kernels: the plan of policy_pass.h with lanes 0 .. 15 of wave 0 as the env lanes, one whole agent (S4) each ---------
// The observations go from those lanes to the policy pass through LDS between workgroup barriers; the action comes back in a register.
// Unlike the path-tracking env's, this env's `done` is real: in the worker rollouts an agent lives in its lane's registers across many
// iterations, falls, is re-drawn keyed (env key, env counter + it) and goes on.

// The prologue of the kernels that start from the env's own state block, behind the policy's registers: the lane's agent (env lanes
// only), and the group's rows of obs_io (16 x 4 floats) into sObs.
__device__ __forceinline__ void resident_prologue(S4& s, bool env_lane, int n, int g0, int i, const float* st, const float* obs_io,
                                                  float* sObs) {
    if (env_lane) s = load(st, n, i);
    const int live = (n - g0 < mlp::GROUP ? n - g0 : mlp::GROUP) * 4;
    if ((int)threadIdx.x < live) sObs[threadIdx.x] = obs_io[(size_t)g0 * 4 + threadIdx.x];
}

// What the env lanes need of a worker rollout's arguments once per iteration.  They rest in LDS and are read where they are used, as
// k_worker_rollout's do (env_path_tracking.hip): held in scalar registers for the whole loop beside the policy's arguments and the
// Philox key schedules derived from them, eight of them were spilled (tools/kernel_resources.py).
struct CpRolloutEnvArgs {
    RingPtrs ring;
    float *st, *obs_io, *act_out;
    uint8_t* done_out;
    uint32_t k0, k1, pk0, pk1;     // env key, the policy's key (exploration noise or draw)
    uint64_t env_ctr, policy_ctr;  // the counters of iteration 0, carried as 64-bit sums
    uint32_t capacity;
    template <class PA>
    __device__ __forceinline__ void park(const PA& pa, float* st_, float* obs_io_, float* act_out_, const RingPtrs& ring_, int capacity_,
                                         uint32_t k0_, uint32_t k1_, uint32_t c1, uint32_t c2, uint8_t* done_out_) {
        ring = ring_;
        st = st_; obs_io = obs_io_; act_out = act_out_; done_out = done_out_;
        k0 = k0_; k1 = k1_; pk0 = pa.k0; pk1 = pa.k1;
        env_ctr = ((uint64_t)c2 << 32) | c1;
        policy_ctr = ((uint64_t)pa.c2 << 32) | pa.c1;
        capacity = (uint32_t)capacity_;
    }
};

// OffPolicyWorker.sample's `iters` iterations (worker.py:91-119: policy -> + N(0, sigma) -> env.step -> ring -> env.reset) for the
// pendulum in ONE launch: `iters` consecutive pairs of mpg_policy_action (k_forward<4, 1, PK, 1>) and k_cp_step_store_reset with the
// noise and env counters and the ring position advancing by one / one / n per pair, each of which fetches the policy's weights or the
// agents' state again.  Per iteration `it` an env lane does what k_cp_step_store_reset does, in its order: ring row (obs, act) at slot
// (next_idx + it * n + i) % capacity, step_agent, (obs2, rew, done), reset_agent if done, and the next observation - into sObs instead
// of obs_out.  (The two worker rollouts each carry these statements: moved into one forced-inline function, the compiler merged the
// two stores of the next observation into one flat store and the kernels' instructions changed.)  State, obs_io, act_out and done_out
// are written after the LAST iteration only (what the chain leaves behind).
// (noise / env) c1, c2: the counters of iteration 0.  The host refuses iters * n > capacity: two iterations would write one ring slot
// from different workgroups.  Everything the chain leaves is bit-identical: the same device functions on the same operands in the same
// order (tests/test_worker_rollout_pendulum_gpu.py).
template <bool PK>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_worker_rollout_pendulum(const cp_policy::Args pa, int n, int iters,
                                                                              float* st, float* obs_io, float* act_out, RingPtrs ring,
                                                                              int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                                              uint32_t c1, uint32_t c2, uint8_t* done_out) {
    __shared__ __attribute__((aligned(16))) float smem[cp_policy::smem_floats<1>()];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 4];
    __shared__ CpRolloutEnvArgs sArg;
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<4, 1> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, 4, 1>(pa, 2, L, w2, r, b3v);
    const int g0 = blockIdx.x * mlp::GROUP, i = g0 + (int)threadIdx.x;
    const bool env_lane = threadIdx.x < mlp::GROUP && i < n;
    S4 s = {};
    resident_prologue(s, env_lane, n, g0, i, st, obs_io, sObs);
    if (threadIdx.x == 0) sArg.park(pa, st, obs_io, act_out, ring, capacity, k0, k1, c1, c2, done_out);
    // the agent's ring slot: (next_idx + it * n + i) % capacity
    uint32_t slot = env_lane ? (uint32_t)(((long)next_idx + i) % capacity) : 0u;
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        mlp::lds_barrier();                              // sObs of this iteration is complete (and the previous pass's LDS is free)
        float a = cp_policy::pass<1>(pa, n, blockIdx.x, sObs, smem, nullptr, L, w2, r, b3v, zmax, saw_nan);
        if (!env_lane) continue;
        const uint64_t nc = sArg.policy_ctr + (uint64_t)it;
        a = cp_policy::explore(a, pa.sigma, i, sArg.pk0, sArg.pk1, (uint32_t)nc, (uint32_t)(nc >> 32), saw_nan);
        write_obs(sArg.ring.obs, slot, s);               // obs before the step
        sArg.ring.act[slot] = a;
        const StepOut o = step_agent(s, a);
        write_obs(sArg.ring.obs2, slot, s);
        sArg.ring.rew[slot] = o.reward;
        sArg.ring.done[slot] = o.done ? 1 : 0;
        if (o.done) {
            const uint64_t ec = sArg.env_ctr + (uint64_t)it;
            s = reset_agent(i, sArg.k0, sArg.k1, (uint32_t)ec, (uint32_t)(ec >> 32));
        }
        if (last) {
            sArg.act_out[i] = a;
            uint8_t* const dn = sArg.done_out;
            if (dn) dn[i] = o.done ? 1 : 0;
            store(sArg.st, n, i, s);
            write_obs(sArg.obs_io, i, s);
        } else {
            write_obs(sObs, threadIdx.x, s);
        }
        slot += (uint32_t)n;
        if (slot >= sArg.capacity) slot -= sArg.capacity;
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// MPGLearner.sample (mpg_learner.py:85-105) for the pendulum in ONE launch: from obs0 take n real-env steps, the first with the replay
// action act0, the later ones with the ONLINE policy's deterministic action; `done` is ignored and nothing is reset.  The stand-alone
// chain is mpg_env_reset_from_obs + n x mpg_env_step + (n - 1) x mpg_policy_action (k_forward<4, 1, PK, 1>, sigma 0) = 2 n launches,
// every policy launch fetching the weights again and every env launch the state.  Here the env lanes form their row's state from obs0
// as k_cp_reset_from_obs does.  The policy is NOT evaluated at step 0 (n - 1 passes, as in the chain, so the status word sees what
// the chain's n - 1 policy launches report and nothing of obs0 itself).  Rewards are written every step at rewards[t * rows + row] (no
// per-lane reward array, no bound on n from it), last_obs after the last step; global memory is read in the prologue only (weights,
// obs0, act0).  Rewards, last observations and the status word are bit-identical to the chain's: the same device functions on the same
// operands in the same order (tests/test_env_rollout_pendulum_gpu.py).
template <bool PK>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_env_rollout_pendulum(const cp_policy::Args pa, int rows, int n,
                                                                           const float* __restrict__ obs0, const float* __restrict__ act0,
                                                                           float* __restrict__ rewards, float* __restrict__ last_obs) {
    __shared__ __attribute__((aligned(16))) float smem[cp_policy::smem_floats<1>()];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 4];
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<4, 1> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, 4, 1>(pa, 2, L, w2, r, b3v);
    const int i = blockIdx.x * mlp::GROUP + (int)threadIdx.x;
    const bool env_lane = threadIdx.x < mlp::GROUP && i < rows;
    S4 s = {};
    float a = 0.f;
    if (env_lane) {                                      // k_cp_reset_from_obs: the state IS the observation
        const float4 o = reinterpret_cast<const float4*>(obs0)[i];
        s = S4{o.x, o.y, o.z, o.w};
        a = act0[i];
    }
    for (int t = 0; t < n; ++t) {
        if (t > 0) {
            mlp::lds_barrier();                          // sObs of step t - 1 is complete (and the previous pass's LDS is free)
            a = cp_policy::pass<1>(pa, rows, blockIdx.x, sObs, smem, nullptr, L, w2, r, b3v, zmax, saw_nan);
        }
        if (!env_lane) continue;
        if (t > 0) a = cp_policy::explore(a, 0.f, i, 0u, 0u, 0u, 0u, saw_nan);   // sigma 0: k_forward's NaN test of the action
        const StepOut o = step_agent(s, a);
        rewards[(size_t)t * rows + i] = o.reward;
        if (t == n - 1) write_obs(last_obs, i, s);
        else write_obs(sObs, threadIdx.x, s);
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// The worker rollout's `iters` iterations for the tanh-squashed Gaussian policy (SAC with an action range, worker.py:96: the action IS
// the sample): `iters` consecutive triples of mpg_normal_fill(n, sample key, sample counter + it), mpg_policy_sample_squashed
// (k_forward<4, 2, PK, 1> and k_row_sums<HeadRow<SquashedHead>>) and k_cp_step_store_reset in ONE launch.  Between the pass and the env step the
// row's two logits come to its env lane through sLogit, the lane draws element i of the iteration's stream and forms a = range *
// tanh(mean + sigma * eps) (cp_policy::sample), which goes to step_agent in a register.
template <bool PK>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_worker_sample_rollout_pendulum(const cp_policy::SampleArgs pa, int n, int iters,
                                                                                     float* st, float* obs_io, float* act_out, RingPtrs ring,
                                                                                     int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                                                     uint32_t c1, uint32_t c2, uint8_t* done_out) {
    __shared__ __attribute__((aligned(16))) float smem[cp_policy::smem_floats<2>()];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 4];
    __shared__ __attribute__((aligned(16))) float sLogit[mlp::GROUP * 2];
    __shared__ CpRolloutEnvArgs sArg;
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<4, 2> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, 4, 2>(pa, 2, L, w2, r, b3v);
    const int g0 = blockIdx.x * mlp::GROUP, i = g0 + (int)threadIdx.x;
    const bool env_lane = threadIdx.x < mlp::GROUP && i < n;
    S4 s = {};
    resident_prologue(s, env_lane, n, g0, i, st, obs_io, sObs);
    if (threadIdx.x == 0) sArg.park(pa, st, obs_io, act_out, ring, capacity, k0, k1, c1, c2, done_out);
    // the agent's ring slot: (next_idx + it * n + i) % capacity
    uint32_t slot = env_lane ? (uint32_t)(((long)next_idx + i) % capacity) : 0u;
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        mlp::lds_barrier();                              // sObs of this iteration is complete (and the previous pass's LDS is free)
        cp_policy::pass<2>(pa, n, blockIdx.x, sObs, smem, sLogit, L, w2, r, b3v, zmax, saw_nan);
        if (!env_lane) continue;
        const uint64_t sc = sArg.policy_ctr + (uint64_t)it;
        const float a = cp_policy::sample(pa, sLogit + 2 * threadIdx.x, i, sArg.pk0, sArg.pk1, (uint32_t)sc, (uint32_t)(sc >> 32));
        write_obs(sArg.ring.obs, slot, s);               // obs before the step
        sArg.ring.act[slot] = a;
        const StepOut o = step_agent(s, a);
        write_obs(sArg.ring.obs2, slot, s);
        sArg.ring.rew[slot] = o.reward;
        sArg.ring.done[slot] = o.done ? 1 : 0;
        if (o.done) {
            const uint64_t ec = sArg.env_ctr + (uint64_t)it;
            s = reset_agent(i, sArg.k0, sArg.k1, (uint32_t)ec, (uint32_t)(ec >> 32));
        }
        if (last) {
            sArg.act_out[i] = a;
            uint8_t* const dn = sArg.done_out;
            if (dn) dn[i] = o.done ? 1 : 0;
            store(sArg.st, n, i, s);
            write_obs(sArg.obs_io, i, s);
        } else {
            write_obs(sObs, threadIdx.x, s);
        }
        slot += (uint32_t)n;
        if (slot >= sArg.capacity) slot -= sArg.capacity;
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// k_eval_rollout_pendulum (below): the env lanes' pointers, resting in LDS as CpRolloutEnvArgs does and for its reason
struct CpEvalEnvArgs {
    float *st, *obs_io, *obs_traj, *act_traj, *rew_traj;
    uint8_t* done_out;
};

// Evaluator.run_n_episodes_parallel's loop (evaluator.py:132-139: compute_mode -> env.step, `done` not consulted, nothing reset) for the
// pendulum in ONE launch: `steps` consecutive pairs of mpg_policy_action (k_forward<4, 1, PK, 1>, sigma 0) and mpg_env_step = 2 * steps
// launches.  Unlike k_env_rollout_pendulum the agents come from the env's own state block and the first observations from obs_io, the
// policy is evaluated at step 0 too (`steps` passes), and the trajectory is recorded: per step t the observation BEFORE the step (out
// of sObs) at obs_traj[(t n + i) 4 ..], the action - unclipped, the env clips its own copy - at act_traj[t n + i] and the reward at
// rew_traj[t n + i].  An agent beyond the done bound keeps stepping, as in the chain.  State, obs_io and the done flags (nullable) are
// written after the LAST step only.  Bit-identical to the chain: the same device functions on the same operands in the same order
// (tests/test_eval_rollout_gpu.py).
template <bool PK>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_eval_rollout_pendulum(const cp_policy::Args pa, int n, int steps, float* st,
                                                                            float* obs_io, float* obs_traj, float* act_traj,
                                                                            float* rew_traj, uint8_t* done_out) {
    __shared__ __attribute__((aligned(16))) float smem[cp_policy::smem_floats<1>()];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 4];
    __shared__ CpEvalEnvArgs sArg;
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<4, 1> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, 4, 1>(pa, 2, L, w2, r, b3v);
    const int g0 = blockIdx.x * mlp::GROUP, i = g0 + (int)threadIdx.x;
    const bool env_lane = threadIdx.x < mlp::GROUP && i < n;
    S4 s = {};
    resident_prologue(s, env_lane, n, g0, i, st, obs_io, sObs);
    if (threadIdx.x == 0) {
        sArg.st = st; sArg.obs_io = obs_io; sArg.obs_traj = obs_traj; sArg.act_traj = act_traj; sArg.rew_traj = rew_traj;
        sArg.done_out = done_out;
    }
    for (int t = 0; t < steps; ++t) {
        mlp::lds_barrier();                              // sObs of this step is complete (and the previous pass's LDS is free)
        float a = cp_policy::pass<1>(pa, n, blockIdx.x, sObs, smem, nullptr, L, w2, r, b3v, zmax, saw_nan);
        if (!env_lane) continue;
        a = cp_policy::explore(a, 0.f, i, 0u, 0u, 0u, 0u, saw_nan);   // sigma 0: k_forward's NaN test of the action
        const size_t row = (size_t)t * (size_t)n + (size_t)i;
        reinterpret_cast<float4*>(sArg.obs_traj)[row] = reinterpret_cast<const float4*>(sObs)[threadIdx.x];   // obs before the step
        sArg.act_traj[row] = a;
        const StepOut o = step_agent(s, a);
        sArg.rew_traj[row] = o.reward;
        if (t == steps - 1) {
            uint8_t* const dn = sArg.done_out;
            if (dn) dn[i] = o.done ? 1 : 0;
            store(sArg.st, n, i, s);
            write_obs(sArg.obs_io, i, s);
        } else {
            write_obs(sObs, threadIdx.x, s);
        }
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// The policy arguments of a launch for OU used outputs - OU = 1: the output activation and the exploration noise; OU = 2: the squashed
// head's constants, `seed` / `ctr` the draw's - and the instantiation that takes them: packed when the weight cache holds W2's image.
// launch(std::bool_constant<PK>, pa) issues the entry point's kernel.
template <int OU, class Launch>
void with_policy_args(const mpg_cfg_t* cfg, const float* policy_params, float explore_sigma, uint64_t seed, uint64_t ctr, Launch&& launch) {
    typename cp_policy::args_of<OU>::type pa;
    pa.params = policy_params;
    pa.pack = mlp::weight_cache_lookup(cfg, mlp::make_net(policy_params, 4, 2).W2, 0);
    pa.status = mpg_status_of(cfg);
    if constexpr (OU == 1) {
        const bool ranged = cfg->action_range > 0.f;       // (as mpg_policy_action forms it: policy_out, host_glue.h)
        pa.out_tanh = (cfg->policy_out_act == MPG_ACT_TANH || ranged) ? 1 : 0;
        pa.out_scale = ranged ? cfg->action_range : 1.f;
        pa.sigma = explore_sigma;
    } else {
        pa.range = cfg->action_range;
        pa.log_r = gauss::log_range(cfg->action_range);
    }
    pa.k0 = (uint32_t)seed; pa.k1 = (uint32_t)(seed >> 32); pa.c1 = (uint32_t)ctr; pa.c2 = (uint32_t)(ctr >> 32);
    for (int i = 0; i < 4; ++i) pa.scale[i] = cfg->obs_scale[i];
    if (pa.pack) launch(std::true_type{}, pa); else launch(std::false_type{}, pa);
}

}  // namespace

// evaluator.py:132-139 for the pendulum: `steps` consecutive pairs mpg_policy_action (explore_sigma 0) + mpg_env_step as one launch
// (k_eval_rollout_pendulum: bit-identical trajectories, state, observations, done flags and status word)
extern "C" int mpg_eval_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int n, int steps, float* state, float* obs_io,
                                         float* obs_traj, float* act_traj, float* rew_traj, uint8_t* done_out, mpg_stream_t stream) {
    if (int rc = env_cfg_refusal("mpg_eval_rollout_pendulum", PENDULUM_ENV, cfg)) return rc;
    if (int rc = eval_rollout_refusal("mpg_eval_rollout_pendulum", n, steps,
                                      policy_params && state && obs_io && obs_traj && act_traj && rew_traj))
        return rc;
    if (int rc = tanh_range_refusal("mpg_eval_rollout_pendulum", cfg)) return rc;
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args<1>(cfg, policy_params, 0.f, 0, 0, [&](auto pk, const auto& pa) {
        hipLaunchKernelGGL(k_eval_rollout_pendulum<decltype(pk)::value>, dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, n, steps, state, obs_io,
                           obs_traj, act_traj, rew_traj, done_out);
    });
    MPG_CHECK_LAUNCH("mpg_eval_rollout_pendulum");
    return MPG_OK;
}

// worker.py:91-119 for the pendulum: `iters` consecutive pairs mpg_policy_action + mpg_env_step_store_reset (noise_ctr + it, ring
// position (next_idx + it * n) % capacity, env_ctr + it) as one launch (k_worker_rollout_pendulum: bit-identical state, observations,
// actions, done flags, ring arrays and status word)
extern "C" int mpg_worker_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                                           float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity,
                                           int next_idx, float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2,
                                           uint8_t* ring_done, uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out, mpg_stream_t stream) {
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    if (int rc = env_cfg_refusal("mpg_worker_rollout_pendulum", PENDULUM_ENV, cfg)) return rc;
    if (int rc = tanh_range_refusal("mpg_worker_rollout_pendulum", cfg)) return rc;
    if (int rc = ring_rollout_refusal("mpg_worker_rollout_pendulum", policy_params && state && obs_io && act_out, n, iters, capacity,
                                      next_idx, ring))
        return rc;
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args<1>(cfg, policy_params, explore_sigma, noise_seed, noise_ctr, [&](auto pk, const auto& pa) {
        mpg_prof_begin(mpg_prof_of(cfg), 2, s);
        hipLaunchKernelGGL(k_worker_rollout_pendulum<decltype(pk)::value>, dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, n, iters, state, obs_io,
                           act_out, ring, capacity, next_idx, MPG_KEY_CTR(env_seed, env_ctr), done_out);
    });
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_rollout_pendulum");
    return MPG_OK;
}

// worker.py:91-119 for the pendulum under the tanh-squashed Gaussian policy: `iters` consecutive triples mpg_normal_fill(n, sample_seed,
// sample_ctr + it) + mpg_policy_sample_squashed + mpg_env_step_store_reset (ring position (next_idx + it * n) % capacity, env_ctr + it) as
// one launch (k_worker_sample_rollout_pendulum: bit-identical state, observations, actions, done flags, ring arrays and status word)
extern "C" int mpg_worker_sample_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state,
                                                  float* obs_io, uint64_t sample_seed, uint64_t sample_ctr, float* act_out, int capacity,
                                                  int next_idx, float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2,
                                                  uint8_t* ring_done, uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out,
                                                  mpg_stream_t stream) {
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    // (the squashed head itself is also built for PathTracking; this launch steps the pendulum)
    if (int rc = env_kind_refusal("mpg_worker_sample_rollout_pendulum", PENDULUM_ENV, cfg)) return rc;
    // what the head asks of a cfg, the widths included (the pointers and the row count are judged below, with the ring)
    if (int rc = gauss::squash_refusal("mpg_worker_sample_rollout_pendulum", cfg, true, 1, 0.f)) return rc;
    if (int rc = ring_rollout_refusal("mpg_worker_sample_rollout_pendulum", policy_params && state && obs_io && act_out, n, iters, capacity,
                                      next_idx, ring))
        return rc;
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args<2>(cfg, policy_params, 0.f, sample_seed, sample_ctr, [&](auto pk, const auto& pa) {
        mpg_prof_begin(mpg_prof_of(cfg), 2, s);
        hipLaunchKernelGGL(k_worker_sample_rollout_pendulum<decltype(pk)::value>, dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, n, iters, state,
                           obs_io, act_out, ring, capacity, next_idx, MPG_KEY_CTR(env_seed, env_ctr), done_out);
    });
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_sample_rollout_pendulum");
    return MPG_OK;
}

// mpg_learner.py:85-105 for the pendulum: mpg_env_reset_from_obs + n x (mpg_policy_action from the second step on, mpg_env_step) as one
// launch (k_env_rollout_pendulum: bit-identical rewards, last observations and status word)
extern "C" int mpg_env_rollout_pendulum(const mpg_cfg_t* cfg, const float* policy_params, int rows, int n, const float* obs0,
                                        const float* act0, float* rewards, float* last_obs, mpg_stream_t stream) {
    if (int rc = env_cfg_refusal("mpg_env_rollout_pendulum", PENDULUM_ENV, cfg)) return rc;
    MPG_REQUIRE(n >= 1, "mpg_env_rollout_pendulum: n >= 1 steps (got %d)", n);
    // (what bounds one launch's run time, as the worker's one-launch samples bound theirs)
    MPG_REQUIRE(n <= 1024, "mpg_env_rollout_pendulum: n <= 1024 steps (got %d)", n);
    MPG_REQUIRE(rows > 0, "mpg_env_rollout_pendulum: no rows (got %d)", rows);
    MPG_REQUIRE(policy_params && obs0 && act0 && rewards && last_obs, "mpg_env_rollout_pendulum: null pointer");
    if (int rc = tanh_range_refusal("mpg_env_rollout_pendulum", cfg)) return rc;
    const int blocks = (rows + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args<1>(cfg, policy_params, 0.f, 0, 0, [&](auto pk, const auto& pa) {
        hipLaunchKernelGGL(k_env_rollout_pendulum<decltype(pk)::value>, dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, rows, n, obs0, act0,
                           rewards, last_obs);
    });
    MPG_CHECK_LAUNCH("mpg_env_rollout_pendulum");
    return MPG_OK;
}

namespace cart_pole {

int reset_from_obs(int n, int obs_dim, float* state, const float* init_obs, hipStream_t s) {
    MPG_REQUIRE(n > 0 && obs_dim == 4 && state && init_obs, "mpg_env_reset_from_obs (cart-pole): bad argument");
    hipLaunchKernelGGL(k_cp_reset_from_obs, dim3((n + 63) / 64), dim3(64), 0, s, n, state, init_obs);
    MPG_CHECK_LAUNCH("k_cp_reset_from_obs");
    return MPG_OK;
}

int reset(int n, int obs_dim, float* state, const uint8_t* done_mask, uint64_t seed, uint64_t ctr, float* obs, hipStream_t s) {
    MPG_REQUIRE(n > 0 && obs_dim == 4 && state && obs, "mpg_env_reset (cart-pole): bad argument");
    hipLaunchKernelGGL(k_cp_reset, dim3((n + 63) / 64), dim3(64), 0, s, n, state, done_mask, MPG_KEY_CTR(seed, ctr), obs);
    MPG_CHECK_LAUNCH("k_cp_reset");
    return MPG_OK;
}

int step(int n, int obs_dim, float* state, const float* action, float* obs, float* reward, uint8_t* done, uint8_t* done_intended,
         hipStream_t s) {
    MPG_REQUIRE(n > 0 && obs_dim == 4 && state && action && obs && reward && done, "mpg_env_step (cart-pole): bad argument");
    hipLaunchKernelGGL(k_cp_step, dim3((n + 63) / 64), dim3(64), 0, s, n, state, action, obs, reward, done, done_intended);
    MPG_CHECK_LAUNCH("k_cp_step");
    return MPG_OK;
}

int step_store_reset(int n, int obs_dim, float* state, const float* action, int capacity, int next_idx, const RingPtrs& ring,
                     uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out, hipStream_t s) {
    MPG_REQUIRE(obs_dim == 4, "mpg_env_step_store_reset (cart-pole): obs_dim");
    hipLaunchKernelGGL(k_cp_step_store_reset, dim3((n + 63) / 64), dim3(64), 0, s, n, state, action, ring, capacity, next_idx,
                       MPG_KEY_CTR(seed, ctr), obs_out, done_out);
    MPG_CHECK_LAUNCH("k_cp_step_store_reset");
    return MPG_OK;
}

}  // namespace cart_pole
