// K1: PathTrackingEnv - vectorised real-environment stepping for gfx950.
//
// One lane per agent; the 20 sub-steps of VehicleDynamics.simulation run in registers, the agent's state
// block is read once and written once (SoA [8][n], coalesced).  The arithmetic follows the reference
// operation-by-operation (envs_and_models/path_tracking_env.py:78-138,144-179,181-199,204-220,410-487):
// this translation unit is compiled with -ffp-contract=off so that every float32 product and sum rounds
// exactly where numpy / TF round it; only the transcendental library calls (sin, cos, atan, tan, log,
// sqrt) differ from the reference's by their last-ulp behaviour.
//
// State block (opaque to callers): v_x, v_y, r, y, phi, x, delta_y, delta_phi.
// Observations carry 6 + K entries, K = num_future_data look-ahead delta-y terms (path_tracking_env.py:385-402).
// env_kind MPG_ENV_INVERTED_PENDULUM is dispatched to env_cart_pole.hip.
#include <type_traits>

#include "env_internal.h"

// The worker's policy pass rides in the env launch (k_policy_step_store_reset, below).  The network engine is compiled here as
// every other translation unit compiles it - contraction allowed - although this file is built with -ffp-contract=off for the
// environment's op-by-op arithmetic: the pragma is lexical, the environment code below is back under "off".
#pragma clang fp contract(fast)
#include "mlp_core.h"
#include "gauss_head.h"
#include "policy_pass.h"

namespace worker_policy {
using namespace mlp;

struct Args {
    const float* params;       // policy network, Keras order
    const float* pack;         // nullable: packed forward image of W2 (weight cache)
    int* status;               // nullable: MPG_STATUS_* word of the caller
    int out_tanh;
    float out_scale, sigma;
    uint32_t k0, k1, c1, c2;   // exploration-noise key and counter
    float scale[8];            // obs_scale (1 beyond obs_dim)
};
// the same for observations with look-ahead entries (obs_dim 7 .. 16: the 16-wide first layer).  A struct of its own: the six-wide
// kernels' arguments stay where they are.
struct WideArgs {
    const float* params;
    const float* pack;
    int* status;
    int out_tanh;
    float out_scale, sigma;
    uint32_t k0, k1, c1, c2;
    int obs_dim;               // the network's actual input width = the row stride of the observations
    float scale[16];           // obs_scale (1 beyond obs_dim)
};
// IN = 6: six-entry observations; IN = 16 stands for "7 .. 16 entries, the actual width is WideArgs::obs_dim" (mlp_core.h)
template <int IN> struct args_of { typedef Args type; };
template <> struct args_of<16> { typedef WideArgs type; };
__device__ __forceinline__ constexpr int obs_dim_of(const Args&) { return 6; }
__device__ __forceinline__ int obs_dim_of(const WideArgs& a) { return a.obs_dim; }

// (OU: the used outputs the pass is built for - two: the deterministic action; four: the Gaussian head's logits)
template <int IN, int OU = 2>
__host__ __device__ constexpr int smem_floats() { return policy_pass::smem_floats<IN, OU>(); }

// One evaluation on the group's observations sObs [16][od] in LDS (policy_pass::stage), the outputs - without noise - to sOut [16][OU]
// (0 beyond `rows`), written by wave 0's own lanes: lane tid < 16 OU forms output tid % OU of row tid / OU.  OU = 2: the action, the
// output activation under the action range.  OU = 4: the logits as policy_logits launches them - the output activation on all four
// columns, no action range (a.out_scale is not read) - formed by lanes 4 row .. 4 row + 3, the lanes that step the row's agent.
template <int IN, int OU>
__device__ __forceinline__ void pass(const typename args_of<IN>::type& a, int rows, long g, const float* sObs, float* smem, float* sOut,
                                     const Lane& L, const float (&w2)[128], const SmallRegs<IN, OU>& r, float b3v, float& zmax,
                                     bool& saw_nan) {
    static_assert(IN == 6 || IN == 16, "these launches are built for six-entry observations and for the 16-wide first layer");
    static_assert(OU == 2 || GROUP * OU == 64, "the four logits of every row of a group are formed by one wave");
    const float pz = policy_pass::stage<IN, OU>(a, rows, g, sObs, smem, L, w2, r, zmax, saw_nan);
    const int tid = threadIdx.x;
    if (tid < GROUP * OU) {
        const int row = tid / OU, o = tid % OU;
        float y = 0.f;
        if (g * GROUP + row < rows) {
            float z = out_preact<out_stride<OU>()>(policy_pass::part_of<IN>(smem), b3v, row, o);
            if constexpr (OU == 2) y = a.out_tanh ? a.out_scale * tanhf(z) : z;
            else y = a.out_tanh ? tanhf(z) : z;
            y += pz;
            saw_nan |= y != y;
        }
        sOut[tid] = y;
    }
}

// The same pass up to the output partials for the kernels that run it ONCE (k_policy_step_store_reset,
// k_policy_sample_step_store_reset): the observations come from global memory, and they are requested BEFORE the weight loads are
// issued (the worker launch's latency is what bench.py times), so policy_pass::load's statements stand here around that fetch.  Leaves
// the lane's bias and row_poison term for the caller's outputs; returns whether the lane's input was NaN.
template <bool PK, int IN, int OU>
__device__ __forceinline__ bool group_forward(const typename args_of<IN>::type& a, int rows, const float* __restrict__ obs, long g,
                                              float* smem, float& b3v, float& pz, float& zmax) {
    constexpr int XSW = xs_of<IN>();
    const int od = obs_dim_of(a);              // a constant at IN = 6
    float* sX = smem + A_IMG;
    const Lane L;
    const Net net = make_net(a.params, od, 4);
    float w2[128];
    SmallRegs<IN, OU> r;
    float xv = 0.f;
    if (threadIdx.x < GROUP * XSW) {           // (columns od .. XSW - 1 stay zero)
        const int row = threadIdx.x / XSW, i = threadIdx.x % XSW;
        const long gr = g * GROUP + row;
        if (gr < rows && i < od) xv = obs[gr * od + i] * a.scale[i];
    }
    b3v = 0.f;
    if (threadIdx.x < GROUP * OU) b3v = net.b3[threadIdx.x % OU];
    load_small<IN, OU>(net, L, r);
    if constexpr (PK) load_w2_packed(a.pack, L, w2); else load_w2_fwd(net.W2, L, w2);
    const bool saw_nan = xv != xv;
    if (threadIdx.x < GROUP * XSW) sX[threadIdx.x] = xv;
    pz = policy_pass::forward<IN, OU>(smem, L, w2, r, zmax);
    return saw_nan;
}

// One 16-row group of mpg_policy_action (tests: native step driver == method-by-method path, tests/test_worker_wide.py).  The group's
// actions, with the exploration noise, go to act_out (global) and to sAct [16][2] for the env lanes of wave 0.
template <bool PK, int IN>
__device__ __forceinline__ void group(const typename args_of<IN>::type& a, int rows, const float* __restrict__ obs, long g, float* smem,
                                      float* sAct, float* __restrict__ act_out) {
    constexpr int OU = 2;
    float b3v, pz, zmax = 0.f;
    bool saw_nan = group_forward<PK, IN, OU>(a, rows, obs, g, smem, b3v, pz, zmax);
    const int tid = threadIdx.x;
    if (tid < GROUP * OU) {
        const int row = (tid / OU) % GROUP, o = tid % OU;
        const long gr = g * GROUP + row;
        float y = 0.f;
        if (gr < rows) {
            float z = out_preact(policy_pass::part_of<IN>(smem), b3v, row, o);
            y = a.out_tanh ? a.out_scale * tanhf(z) : z;
            y += pz;
            if (a.sigma > 0.f) {   // OffPolicyWorker.sample: action += N(0, sigma), worker.py:97-98
                Philox4 p = philox4x32_10((uint32_t)gr, a.c1, a.c2, 0x5eedu + (uint32_t)o, a.k0, a.k1);
                float u1 = u01(p.v[0]), u2 = u01(p.v[1]);
                y = add_gauss_noise(y, a.sigma, u1, u2);
            }
            saw_nan |= y != y;
            act_out[gr * OU + o] = y;
        }
        sAct[tid] = y;
    }
    report_activation_range(a.status, zmax);
    if (a.status && saw_nan) atomicOr(a.status, MPG_STATUS_NAN);
}

// One 16-row group of mpg_policy_sample on the worker's own draw: the four logits of every row, then k_row_sums<HeadRow<PlainHead>>'s row body
// (gauss::gauss_row) on eps = elements 2 gr, 2 gr + 1 of the stream mpg_normal_fill writes for (a.k0 .. a.c2).  The logits go through
// sLogit [16][4] to the first of the row's four lanes, which draws, samples and leaves the action in act_out, the log-density in
// logp_out (nullable) and the action in sAct [16][2] for the env lanes: LDS is in order within a wave.  a.sigma is not read.
template <bool PK, int IN>
__device__ __forceinline__ void sample_group(const typename args_of<IN>::type& a, int rows, const float* __restrict__ obs, long g,
                                             float* smem, float* sLogit, float* sAct, float* __restrict__ act_out,
                                             float* __restrict__ logp_out) {
    constexpr int OU = 4;
    float b3v, pz, zmax = 0.f;
    bool saw_nan = group_forward<PK, IN, OU>(a, rows, obs, g, smem, b3v, pz, zmax);
    const int tid = threadIdx.x;
    if (tid < GROUP * OU) {
        const int row = tid / OU, o = tid % OU;
        const long gr = g * GROUP + row;
        float y = 0.f;
        if (gr < rows) {
            float z = out_preact<out_stride<OU>()>(policy_pass::part_of<IN>(smem), b3v, row, o);
            y = a.out_tanh ? tanhf(z) : z;
            y += pz;
            saw_nan |= y != y;
        }
        sLogit[tid] = y;
        __builtin_amdgcn_wave_barrier();
        if (o == 0) {
            float act[2] = {0.f, 0.f};
            if (gr < rows) {
                float eps[2];
                gauss::normal_pair((uint32_t)(gr >> 1), (int)(gr & 1), a.k0, a.k1, a.c1, a.c2, eps[0], eps[1]);
                const float lp = gauss::gauss_row(2, sLogit + row * OU, eps, act);
                act_out[gr * 2] = act[0];
                act_out[gr * 2 + 1] = act[1];
                if (logp_out) logp_out[gr] = lp;
            }
            sAct[2 * row] = act[0];
            sAct[2 * row + 1] = act[1];
        }
    }
    report_activation_range(a.status, zmax);
    if (a.status && saw_nan) atomicOr(a.status, MPG_STATUS_NAN);
}

// The exploration noise of `group` for a kernel that calls pass() (k_worker_rollout, below): lane tid < 32 of wave 0 takes its own
// action back out of sAct, adds N(0, sigma) from the same Philox draw as `group` - row gr, output o, the 64-bit counter (c1, c2) -
// tests the sum for NaN as `group` does (pass() tested the action before the noise: a NaN there is a NaN here) and puts it back for
// the env lanes: LDS is in order within a wave.  Returns the action (0 beyond `rows`, as in sAct).
__device__ __forceinline__ float explore(float sigma, int rows, long g, float* sAct, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2,
                                         bool& saw_nan) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));              // (opaque: the lane's predicate is formed here, not held across the caller's loop)
    const int row = (tid / 2) % GROUP, o = tid % 2;
    const long gr = g * GROUP + row;
    float y = sAct[tid];
    if (gr < rows && sigma > 0.f) {   // OffPolicyWorker.sample: action += N(0, sigma), worker.py:97-98
        Philox4 p = philox4x32_10((uint32_t)gr, c1, c2, 0x5eedu + (uint32_t)o, k0, k1);
        float u1 = u01(p.v[0]), u2 = u01(p.v[1]);
        y = add_gauss_noise(y, sigma, u1, u2);
        saw_nan |= y != y;
        sAct[tid] = y;
    }
    return y;
}
// Row gr's action from its four logits l[4] (mean | log-std), by the first of the row's four lanes: elements 2 gr and 2 gr + 1 of the
// stream mpg_normal_fill(2 n, key, counter (c1, c2)) writes - sample_group's draw - and k_row_sums<HeadRow<PlainHead>>'s row body, or with SQ
// k_row_sums<HeadRow<SquashedHead>>'s (gauss::squash_row under `range` and the host-formed log_r).  The log-density is not kept: the worker
// discards it and the ring has no column for it.
template <bool SQ>
__device__ __forceinline__ void sample_act(const float* l, long gr, float range, float log_r, uint32_t k0, uint32_t k1, uint32_t c1,
                                           uint32_t c2, float (&act)[2]) {
    float eps[2];
    gauss::normal_pair((uint32_t)(gr >> 1), (int)(gr & 1), k0, k1, c1, c2, eps[0], eps[1]);
    // The row body, one component per call (ad = 1 on {mean_k, log_std_k} and eps_k): the bodies are sums over independent components,
    // and the log-density, which joins them, is dead here.  Called on the whole row (ad = 2) the squashed instantiations had scratch
    // (tools/kernel_resources.py); this form has none.
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float lk[2] = {l[k], l[2 + k]};
        if constexpr (SQ) gauss::squash_row(1, range, log_r, lk, eps + k, act + k);
        else gauss::gauss_row(1, lk, eps + k, act + k);
        __builtin_amdgcn_sched_barrier(0);
    }
}
}  // namespace worker_policy
#pragma clang fp contract(off)

// the MPC baseline's solve, for k_mpc_rollout at the end of this file (the header is under "off" itself)
#include "mpc_core.h"

namespace {

#ifdef MPG_TIMELINE   // diagnostic build only (tools/timeline.sh)
__device__ unsigned long long g_env_tl[2][16];
#define ENV_TL(k) do { __builtin_amdgcn_sched_barrier(0); if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == 200)) g_env_tl[blockIdx.x ? 1 : 0][k] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define ENV_TL(k)
#endif

constexpr float PI_F = 3.14159265358979323846f;          // float32(np.pi)
constexpr float TWO_PI_F = (float)(2.0 * 3.14159265358979323846);   // float32(2*np.pi)
constexpr float PERIOD = 1200.f;                          // path_tracking_env.py:205

// vehicle parameters, path_tracking_env.py:60-68 (cast to float32 like :86-93)
constexpr float C_f = -128915.5f, C_r = -85943.6f, A_ = 1.06f, B_ = 1.85f, MASS = 1412.f, I_z = 1536.7f,
                MIU = 1.0f, G_ = 9.81f;
// f_xu's constants, :95-101,135-136: the axle loads and the products with tau = 1/base_freq (a python float, cast on contact, :141)
constexpr float F_zf = B_ * MASS * G_ / (A_ + B_), F_zr = A_ * MASS * G_ / (A_ + B_);
constexpr float tau = 0.005f;
constexpr float K1 = tau * (A_ * C_f - B_ * C_r);
constexpr float K2 = tau * C_f, K3 = tau * MASS, K4 = tau * (C_f + C_r);
constexpr float K5 = (tau * A_) * C_f;
constexpr float K6 = tau * ((A_ * A_) * C_f + (B_ * B_) * C_r);

struct PathRef {
    float y, phi;
};

// sin and cos of a bounded argument (headings within +-pi, path phases below 38 rad) without the library routine's
// large-argument machinery: three-term Cody-Waite reduction by pi/2 (k * 1.5703125 is exact for |k| < 2^8), then the
// minimax polynomials of the Cephes single-precision kernels on [-pi/4, pi/4].  Measured against float64 on 4M draws
// each of [-3.3, 3.3], [0, 38] and [-200, 200]: absolute error <= 9.2e-8 for both (numpy's float32 sin/cos: 8.5e-8);
// the results only ever enter sums with O(1) terms.  ~25 instructions for both, against ~110 for sincosf - the env
// kernel spends most of its time in the 20 + 3 of them per step.  |a| > 200 (a caller's own far-away x) takes sincosf.
__device__ __forceinline__ void sincos_bounded(float a, float& s, float& c) {
    if (fabsf(a) > 200.f) {
        sincosf(a, &s, &c);
        return;
    }
    const float kf = rintf(a * 0.63661977236758134308f);            // a * 2/pi
    float r = fmaf(-kf, 1.5703125f, a);
    r = fmaf(-kf, 4.837512969970703125e-4f, r);
    r = fmaf(-kf, 7.54978995489188216e-8f, r);
    const float z = r * r;
    const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f) * z, r, r);
    const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f) * z, z,
                          fmaf(-0.5f, z, 1.f));
    const int q = (int)kf;
    const float ss = (q & 1) ? pc : ps, cc = (q & 1) ? ps : pc;
    s = (q & 2) ? -ss : ss;
    c = ((q + 1) & 2) ? -cc : cc;
}

// ReferencePath.compute_path_y / compute_path_phi, path_tracking_env.py:207-220.
// numpy evaluates (x - shift) * 2 * np.pi / T in float32, one rounding per operator; y and the slope are
// accumulated curve by curve into a float32 zero array.
__device__ __forceinline__ PathRef path_ref(float x) {
    const float Amp[3] = {7.5f, 2.5f, -5.f};
    const float T[3] = {200.f, 300.f, 400.f};
    float y = 0.f, d = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float arg = (((x - 0.f) * 2.f) * PI_F) / T[i];
        float s, c;
        sincos_bounded(arg, s, c);
        y = y + Amp[i] * s;
        // magnitude * 2 * np.pi / T is a python-float (double) scalar, rounded once when it meets the array
        const float k = (float)((double)Amp[i] * 2.0 * 3.14159265358979323846 / (double)T[i]);
        d = d + k * c;
    }
    PathRef r;
    r.y = y;
    r.phi = atanf(d);
    return r;
}

// x / 200.f, correctly rounded, in three instructions instead of the ~12 of an IEEE division: q = RN(x * RN(1/200)), the
// exact remainder by one fma, one correction fma (Markstein).  Checked against the division on every float32 of 30 binades
// (2^-17 .. 2^12, 2.5e8 values, no mismatch; outside the denormal range the mantissa behaviour does not depend on the
// binade).  Three of the five divisions of a sub-step are by 200.
__device__ __forceinline__ float div200(float x) {
    const float c = 0.005f;                    // RN(1/200)
    const float q = x * c;
    const float r = fmaf(-q, 200.f, x);
    return fmaf(r, c, q);
}

__device__ __forceinline__ float wrap_pi(float a) {        // :168-169 / :176-177
    if (a > PI_F) a = a - TWO_PI_F;
    if (a <= -PI_F) a = a + TWO_PI_F;
    return a;
}

__global__ void __launch_bounds__(64) k_reset_from_obs(int n, int od, float* __restrict__ st, const float* __restrict__ obs) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* o = obs + (size_t)i * od;                                            // only the six base entries are read
    float vx = o[0] + 20.f, vy = o[1], r = o[2], dy = o[3], dphi = o[4], x = o[5];   // _get_state :404-408
    PathRef p = path_ref(x);                                                          // :415-417
    st[0 * (size_t)n + i] = vx;
    st[1 * (size_t)n + i] = vy;
    st[2 * (size_t)n + i] = r;
    st[3 * (size_t)n + i] = dy + p.y;      // :420
    st[4 * (size_t)n + i] = dphi + p.phi;  // :419 (no wrap here, as in the reference)
    st[5 * (size_t)n + i] = x;
    st[6 * (size_t)n + i] = dy;
    st[7 * (size_t)n + i] = dphi;
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    float u1 = u01(a), u2 = u01(b);
    float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincos_bounded(TWO_PI_F * u2, s, c);                  // argument in [0, 2 pi)
    z0 = rad * c;
    z1 = rad * s;
}

struct Agent {   // one agent's state block in registers
    float vx, vy, r, y, phi, x, dy, dphi;
};

__device__ __forceinline__ Agent load_agent(const float* __restrict__ st, size_t N, int i) {
    Agent a;
    a.vx = st[0 * N + i]; a.vy = st[1 * N + i]; a.r = st[2 * N + i]; a.y = st[3 * N + i];
    a.phi = st[4 * N + i]; a.x = st[5 * N + i]; a.dy = st[6 * N + i]; a.dphi = st[7 * N + i];
    return a;
}
__device__ __forceinline__ void store_agent(float* __restrict__ st, size_t N, int i, const Agent& a) {
    st[0 * N + i] = a.vx; st[1 * N + i] = a.vy; st[2 * N + i] = a.r; st[3 * N + i] = a.y;
    st[4 * N + i] = a.phi; st[5 * N + i] = a.x; st[6 * N + i] = a.dy; st[7 * N + i] = a.dphi;
}
// ReferencePath.compute_path_y alone (the look-ahead terms need no heading)
__device__ __forceinline__ float path_y_only(float x) {
    const float Amp[3] = {7.5f, 2.5f, -5.f};
    const float T[3] = {200.f, 300.f, 400.f};
    float y = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) y = y + Amp[i] * sinf((((x - 0.f) * 2.f) * PI_F) / T[i]);
    return y;
}

// _get_obs, path_tracking_env.py:385-402: [v_x - 20, v_y, r, delta_y, delta_phi, x | K look-ahead delta-y terms].
// od = 6 + K.  The look-ahead abscissa advances by v_x * 1. / 200 * 20 * 2 per entry (float32, operator by operator,
// :394-395) and is NOT wrapped to the path period; y is the vehicle's current world-frame y.
__device__ __forceinline__ void write_obs(float* __restrict__ obs, int i, int od, const Agent& a) {
    if (od == 6) {
        float2* o = reinterpret_cast<float2*>(obs + (size_t)i * 6);
        o[0] = make_float2(a.vx - 20.f, a.vy);
        o[1] = make_float2(a.r, a.dy);
        o[2] = make_float2(a.dphi, a.x);
        return;
    }
    float* o = obs + (size_t)i * od;
    o[0] = a.vx - 20.f; o[1] = a.vy; o[2] = a.r; o[3] = a.dy; o[4] = a.dphi; o[5] = a.x;
    float x_ = a.x;
    const float adv = (((a.vx * 1.f) / 200.f) * 20.f) * 2.f;
    for (int k = 6; k < od; ++k) {
        x_ = x_ + adv;
        o[k] = a.y - path_y_only(x_);
    }
}

// PathTrackingEnv.reset() for one agent, path_tracking_env.py:423-454, on the Philox stream (i, ctr)
__device__ __forceinline__ void reset_agent(Agent& ag, int i, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2) {
    Philox4 a = philox4x32_10((uint32_t)i, c1, c2, 0u, k0, k1);
    Philox4 b = philox4x32_10((uint32_t)i, c1, c2, 1u, k0, k1);
    float x = 600.f * u01(a.v[0]);                    // :426
    float vx = 15.f + 10.f * u01(a.v[1]);             // :434
    float z0, z1, z2, z3;
    box_muller(a.v[2], a.v[3], z0, z1);
    box_muller(b.v[0], b.v[1], z2, z3);
    float dy = z0;                                     // :428
    float dphi = z1 * (float)(3.14159265358979323846 / 9.0);   // :431
    float beta = z2 * 0.15f;                           // :435
    float r = z3 * 0.3f;                               // :437
    PathRef p = path_ref(x);
    float y = dy + p.y;                                // compute_y :222-224
    float phi = wrap_pi(dphi + p.phi);                 // compute_phi :230-235
    float sb, cb;                                       // beta = 0.15 * N(0, 1): far inside the bounded range
    sincos_bounded(beta, sb, cb);
    ag.vx = vx; ag.vy = vx * (sb / cb);                // :436, tan(beta)
    ag.r = r; ag.y = y; ag.phi = phi; ag.x = x;
    ag.dy = y - p.y;                                   // :450
    ag.dphi = phi - p.phi;                             // :449
}

struct StepOut {
    float reward;
    bool done, done_intended;
};

// PathTrackingEnv.step for one agent (:456-487): reward on the pre-step state, 20 sub-steps, done flags.  The sub-steps come in two
// forms that perform the same float32 operations on the same operands in the same order per variable, so their results are
// bit-identical; everything around them is stated once.
// LANES = 1: one lane per agent runs the sub-steps one after the other (q and sc are not used).
// LANES = 4: four lanes per agent (lanes 4a .. 4a+3 of one wave, q = lane & 3).  The sub-steps' serial part is the planar dynamics
// (v_x, v_y, r) and the heading; the sincos of each heading and the world-frame increments are not on that chain and delta_y /
// delta_phi only matter after the last sub-step.  So: (A) every lane runs the short serial chain and the 20 (heading, v_x, v_y)
// triples go to LDS, (B) lane q evaluates the increments of sub-steps q, q+4, .. (5 of the 20 sincos each), (C) every lane adds the
// increments in order: ~2450 instead of ~4300 instructions per wave, and 256 waves instead of 64 for 4096 agents.  sc: this agent's
// 100 floats of LDS, [5][20].
template <int LANES>
__device__ __forceinline__ StepOut step_agent(Agent& ag, const float2 an, const int q = 0, float* sc = nullptr) {
    static_assert(LANES == 1 || LANES == 4, "one lane or four lanes per agent");
    StepOut out;
    float vx = ag.vx, vy = ag.vy, r = ag.r, y = ag.y, phi = ag.phi, x = ag.x, dy = ag.dy, dphi = ag.dphi;
    // step(): scale and clip the action, path_tracking_env.py:457-459
    const float ACT_HI0 = (float)(1.2 * 3.14159265358979323846 / 9.0), ACT_HI1 = 3.f;
    float steer = ((an.x * 1.2f) * PI_F) / 9.f;
    float a_x = an.y * 3.f;
    steer = fminf(fmaxf(steer, -ACT_HI0), ACT_HI0);
    a_x = fminf(fmaxf(a_x, -ACT_HI1), ACT_HI1);

    // compute_rewards on the PRE-step veh_state, :181-199
    {
        float t = vx - 20.f;
        float devi_v = -(t * t), devi_y = -(dy * dy), devi_phi = -(dphi * dphi), p_yaw = -(r * r),
              p_steer = -(steer * steer), p_ax = -(a_x * a_x);
        out.reward = 0.01f * devi_v + 0.04f * devi_y + 0.1f * devi_phi + 0.02f * p_yaw + 5.f * p_steer + 0.05f * p_ax;
    }

    // f_xu pieces that depend on the action only, :95-101,135-136
    const float F_xf = a_x < 0.f ? MASS * a_x / 2.f : 0.f;
    const float F_xr = a_x < 0.f ? MASS * a_x / 2.f : MASS * a_x;
    const float miu_f = sqrtf((MIU * F_zf) * (MIU * F_zf) - F_xf * F_xf) / F_zf;
    const float miu_r = sqrtf((MIU * F_zr) * (MIU * F_zr) - F_xr * F_xr) / F_zr;

    // simulation(), :144-179.  delta_y / delta_phi are overwritten by every sub-step, so the reference path is evaluated once,
    // for the last one.
    float vx_pre = vx, vy_pre = vy, r_pre = r;  // state entering the LAST sub-step (for `others`)
    float x_u = x, phi_u = phi;                 // x and phi of the last sub-step before their wraps (:163-165)
    if constexpr (LANES == 1) {
        // The loop is deliberately NOT unrolled: one wave per CU runs this kernel, once per launch, with a cold instruction cache -
        // 20 unrolled sub-steps (7300 instructions, 58 KB) spent more time fetching code than executing it (18.5 us -> 22 us when
        // the unrolled body was made cheaper; measured).
#pragma unroll 1
        for (int s = 0; s < 20; ++s) {
            vx_pre = vx; vy_pre = vy; r_pre = r;
            // prediction -> f_xu with tau = 1/200 on (v_x, v_y, r); entries 3-5 are overwritten below
            float nvx = vx + tau * (a_x + vy * r);
            float nvy = (((MASS * vy) * vx + K1 * r) - (K2 * steer) * vx - (K3 * (vx * vx)) * r) / (MASS * vx - K4);
            float nr = ((((-I_z) * r) * vx - K1 * vy) + (K5 * steer) * vx) / (K6 - I_z * vx);
            nvx = fminf(fmaxf(nvx, 1.f), 35.f);     // :153
            // world frame, :156-160: phi first, then y and x with the OLD v_x, v_y but the NEW phi (view aliasing)
            phi = phi + div200(r);
            float sp, cp;
            sincos_bounded(phi, sp, cp);
            y = y + div200(vx * sp + vy * cp);
            x = x + div200(vx * cp - vy * sp);
            vx = nvx; vy = nvy; r = nr;             // :161
            x_u = x; phi_u = phi;                   // :163-165 read x and phi before their wraps
            phi = wrap_pi(phi);                     // :168-169
            if (x > PERIOD) x = x - PERIOD;         // :171
            if (x <= 0.f) x = x + PERIOD;           // :172
        }
    } else {
        ENV_TL(2);
#pragma unroll 1
        for (int s = 0; s < 20; ++s) {              // (A) dynamics and heading
            vx_pre = vx; vy_pre = vy; r_pre = r;
            float nvx = vx + tau * (a_x + vy * r);
            float nvy = (((MASS * vy) * vx + K1 * r) - (K2 * steer) * vx - (K3 * (vx * vx)) * r) / (MASS * vx - K4);
            float nr = ((((-I_z) * r) * vx - K1 * vy) + (K5 * steer) * vx) / (K6 - I_z * vx);
            nvx = fminf(fmaxf(nvx, 1.f), 35.f);     // :153
            phi = phi + div200(r);                  // :156, the OLD yaw rate
            if ((s & 3) == q) { sc[s] = phi; sc[20 + s] = vx; sc[40 + s] = vy; }   // new heading, OLD velocities (:157-160)
            phi_u = phi;
            vx = nvx; vy = nvy; r = nr;             // :161
            phi = wrap_pi(phi);                     // :168-169
        }
        __builtin_amdgcn_wave_barrier();            // the four lanes of an agent sit in one wave: LDS is in order within it
        ENV_TL(3);
#pragma unroll 1
        for (int s = q; s < 20; s += 4) {           // (B) this lane's five sub-steps
            float sp, cp;
            sincos_bounded(sc[s], sp, cp);
            const float ovx = sc[20 + s], ovy = sc[40 + s];
            sc[60 + s] = div200(ovx * sp + ovy * cp);
            sc[80 + s] = div200(ovx * cp - ovy * sp);
        }
        __builtin_amdgcn_wave_barrier();
        ENV_TL(4);
#pragma unroll 1
        for (int s4 = 0; s4 < 20; s4 += 4) {        // (C) positions, in order; four increments per LDS round trip
            const float4 iy = *reinterpret_cast<const float4*>(sc + 60 + s4), ix = *reinterpret_cast<const float4*>(sc + 80 + s4);
            const float ay[4] = {iy.x, iy.y, iy.z, iy.w}, ax[4] = {ix.x, ix.y, ix.z, ix.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                y = y + ay[u];
                x = x + ax[u];
                x_u = x;                            // :163-164 read x before the wrap
                if (x > PERIOD) x = x - PERIOD;     // :171
                if (x <= 0.f) x = x + PERIOD;       // :172
            }
        }
    }
    ENV_TL(5);
    {
        PathRef p = path_ref(x_u);              // :163-164
        dphi = wrap_pi(phi_u - p.phi);          // :165, :176-177
        dy = y - p.y;                           // :166
    }
    ENV_TL(6);

    // `others` of the last sub-step (:100-101,135-138), judge_done :474-487
    const float alpha_f = atanf((vy_pre + A_ * r_pre) / vx_pre) - steer;
    const float alpha_r = atanf((vy_pre - B_ * r_pre) / vx_pre);
    const float afb = 3.f * miu_f * F_zf / C_f, arb = 3.f * miu_r * F_zr / C_r;
    const float rb = miu_r * G_ / fabsf(vx_pre);
    const bool geo = (fabsf(dy) > 3.f) | (fabsf(dphi) > PI_F / 4.f) | (vx < 2.f);
    const bool lit = geo | (alpha_f < -afb) | (alpha_f > afb) | (alpha_r < -arb) | (alpha_r > arb) | (r < -rb) |
                     (r > rb);
    out.done = lit;
    out.done_intended = geo | (fabsf(alpha_f) > fabsf(afb)) | (fabsf(alpha_r) > fabsf(arb)) | (fabsf(r) > rb);

    ag.vx = vx; ag.vy = vy; ag.r = r; ag.y = y; ag.phi = phi; ag.x = x; ag.dy = dy; ag.dphi = dphi;
    return out;
}

__global__ void __launch_bounds__(64) k_reset(int n, float* __restrict__ st, const uint8_t* __restrict__ mask,
                                              uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2,
                                              float* __restrict__ obs, int od) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Agent ag = load_agent(st, n, i);
    if (mask == nullptr || mask[i]) {
        reset_agent(ag, i, k0, k1, c1, c2);
        store_agent(st, n, i, ag);
    }
    write_obs(obs, i, od, ag);
}

__global__ void __launch_bounds__(64) k_step(int n, float* __restrict__ st, const float* __restrict__ action,
                                             float* __restrict__ obs, float* __restrict__ reward,
                                             uint8_t* __restrict__ done, uint8_t* __restrict__ done_intended, int od) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Agent ag = load_agent(st, n, i);
    const StepOut o = step_agent<1>(ag, reinterpret_cast<const float2*>(action)[i]);
    reward[i] = o.reward;
    done[i] = o.done ? 1 : 0;
    if (done_intended) done_intended[i] = o.done_intended ? 1 : 0;
    store_agent(st, n, i, ag);
    write_obs(obs, i, od, ag);
}

// The next minibatch draw, gathered by spare workgroups of the env launch (mpg_env_step_store_reset_draw): one lane per
// drawn row, the same Philox draw as k_target_fused / k_sample_gather; rows whose slot the env lanes are writing are left
// to the consumer.
struct PreDraw {
    int rows, n_storage, env_blocks;
    uint32_t k0, k1, c1, c2;
    int* o_idx;
    float *o_obs, *o_act, *o_rew, *o_obs2, *o_done;
};
__device__ __forceinline__ void predraw_row(const PreDraw& d, const RingPtrs& ring, int capacity, int fresh_start, int fresh_count,
                                            int gr) {
    const Philox4 p = philox4x32_10((uint32_t)(gr >> 2), d.c1, d.c2, 0x1d5u, d.k0, d.k1);
    const long sr = (long)(((uint64_t)philox_word(p, gr & 3) * (uint64_t)d.n_storage) >> 32);
    int off = (int)sr - fresh_start;
    if (off < 0) off += capacity;
    if (off < fresh_count) return;
    float o1[6], o2[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) { o1[i] = ring.obs[sr * 6 + i]; o2[i] = ring.obs2[sr * 6 + i]; }
    const float2 ac = reinterpret_cast<const float2*>(ring.act)[sr];
    const float rw = ring.rew[sr];
    const uint8_t dn = ring.done[sr];
    if (d.o_idx) d.o_idx[gr] = (int)sr;
#pragma unroll
    for (int i = 0; i < 6; ++i) { d.o_obs[(long)gr * 6 + i] = o1[i]; d.o_obs2[(long)gr * 6 + i] = o2[i]; }
    reinterpret_cast<float2*>(d.o_act)[gr] = ac;
    d.o_rew[gr] = rw;
    if (d.o_done) d.o_done[gr] = (float)dn;
}
// The spare workgroups of an env launch, the blocks from pd.env_blocks on, of NT threads each (the launch's block size, a template
// argument: as a run-time one it changed the gather's address arithmetic): one drawn row per thread.  Returns whether this block
// is one of them (it has then done its work and the kernel returns).
template <int NT>
__device__ __forceinline__ bool predraw_block(const PreDraw& pd, const RingPtrs& ring, int capacity, int fresh_start, int fresh_count) {
    if ((int)blockIdx.x < pd.env_blocks) return false;
    const int gr = ((int)blockIdx.x - pd.env_blocks) * NT + threadIdx.x;
    if (gr < pd.rows) predraw_row(pd, ring, capacity, fresh_start, fresh_count, gr);
    return true;
}

// OffPolicyWorker.sample's inner body after the policy (worker.py:108-112) for agent i, whose state `ag` and action `an` the caller
// has read: the transition (obs, action, RAW reward, obs', done) written straight into the replay ring slot (next_idx + i) % capacity
// (buffer.py:46-55) around env.step, then env.reset() if the agent is done (path_tracking_env.py:445), its state and its next
// observation.  LANES = 4: lane q of the agent's four (step_agent<4>; sc: the agent's LDS) does the q-th share of the stores.
// LANES = 1: the one lane stores everything.
template <int LANES>
__device__ __forceinline__ void env_lane(Agent ag, const float2 an, int n, int i, int q, float* sc, float* st, const RingPtrs& ring,
                                         int capacity, int next_idx, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2, float* obs_out,
                                         uint8_t* done_out, int od) {
    const size_t slot = (size_t)((next_idx + i) % capacity);
    if (LANES == 1 || q == 0) {
        write_obs(ring.obs, (int)slot, od, ag);                 // obs before the step
        reinterpret_cast<float2*>(ring.act)[slot] = an;
    }
    ENV_TL(1);
    const StepOut o = step_agent<LANES>(ag, an, q, sc);
    ENV_TL(7);
    if (LANES == 1 || q == 1) {
        write_obs(ring.obs2, (int)slot, od, ag);
        ring.rew[slot] = o.reward;
        ring.done[slot] = o.done ? 1 : 0;
        if (done_out) done_out[i] = o.done ? 1 : 0;
    }
    if (o.done) reset_agent(ag, i, k0, k1, c1, c2);
    if (LANES == 1 || q == 2) store_agent(st, n, i, ag);
    if (LANES == 1 || q == 3) write_obs(obs_out, i, od, ag);
    ENV_TL(8);
}

// env_lane with four lanes per agent: the latency form (256 waves instead of 64 for 4096 agents).  Blocks beyond the env lanes'
// gather the draw (pd.rows > 0).
__global__ void __launch_bounds__(64) k_step_store_reset(int n, float* __restrict__ st, const float* __restrict__ action,
                                                         RingPtrs ring, int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                         uint32_t c1, uint32_t c2, float* __restrict__ obs_out,
                                                         uint8_t* __restrict__ done_out, int od, PreDraw pd) {
    if (pd.rows > 0 && predraw_block<64>(pd, ring, capacity, next_idx, n)) return;
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    ENV_TL(0);
    const int t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2, q = t & 3;
    if (i >= n) return;
    const Agent ag = load_agent(st, n, i);
    const float2 an = reinterpret_cast<const float2*>(action)[i];
    env_lane<4>(ag, an, n, i, q, s_quad + (threadIdx.x >> 2) * 100, st, ring, capacity, next_idx, k0, k1, c1, c2, obs_out, done_out, od);
}

// The same launch with ONE lane per agent (step_agent<1>, like k_step): the four-lane form above buys latency at 4096 agents (256 waves
// instead of 64 on 256 CUs) at the price of ~2.3x the instructions per agent; from MPG_ENV_ONE_LANE_FROM agents on the chip is full either
// way and the instruction count is what is left (2^20 agents: 264 us four-lane against k_step's 61).  The two forms are bit-identical
// (step_agent; tests/test_env_gpu.py compares fused and separate calls at both sizes).
constexpr int MPG_ENV_ONE_LANE_FROM = 65536;
__global__ void __launch_bounds__(64) k_step_store_reset_1(int n, float* __restrict__ st, const float* __restrict__ action,
                                                           RingPtrs ring, int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                           uint32_t c1, uint32_t c2, float* __restrict__ obs_out,
                                                           uint8_t* __restrict__ done_out, int od, PreDraw pd) {
    if (pd.rows > 0 && predraw_block<64>(pd, ring, capacity, next_idx, n)) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Agent ag = load_agent(st, n, i);
    const float2 an = reinterpret_cast<const float2*>(action)[i];
    env_lane<1>(ag, an, n, i, 0, nullptr, st, ring, capacity, next_idx, k0, k1, c1, c2, obs_out, done_out, od);
}

// The env tail of the two launches below: the group's policy pass has left the actions in sAct [16][2]; wave 0, four lanes per agent,
// steps the group's 16 agents with env_lane<4> (it wrote sAct itself: LDS is in order within a wave).  The other waves are done.
__device__ __forceinline__ void group_env_lanes(int n, int od, float* __restrict__ st, float* __restrict__ obs_io, const float* sAct,
                                                float* s_quad, const RingPtrs& ring, int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                uint32_t c1, uint32_t c2, uint8_t* __restrict__ done_out) {
    if (threadIdx.x >= 64) return;
    __builtin_amdgcn_wave_barrier();
    const int i = blockIdx.x * mlp::GROUP + (threadIdx.x >> 2), q = threadIdx.x & 3;
    if (i >= n) return;
    const Agent ag = load_agent(st, n, i);
    const float2 an = make_float2(sAct[2 * (threadIdx.x >> 2)], sAct[2 * (threadIdx.x >> 2) + 1]);
    env_lane<4>(ag, an, n, i, q, s_quad + (threadIdx.x >> 2) * 100, st, ring, capacity, next_idx, k0, k1, c1, c2, obs_io, done_out, od);
}

// OffPolicyWorker.sample's whole inner body (worker.py:95-112) in ONE launch: the policy pass of a 16-agent group by a 512-thread
// workgroup, then env_lane<4> for those 16 agents on wave 0.  The stand-alone pair is two launches of one wave per CU each (7 + 14 us
// at 4096 agents); fused, the env lanes start the moment their group's actions exist.  Blocks beyond the policy groups gather the
// minibatch about to be drawn (predraw_block).
// IN = 6: six-entry observations.  IN = 16: observations with look-ahead entries (obs_dim 7 .. 16 = pa.obs_dim, the row stride of
// obs_io and of the ring's observation arrays) on the 16-wide first layer; these instantiations gather no draw (predraw_row is
// six-wide, and the gradient launch that would consume the rows does not exist at these widths): their grid is the policy groups
// and pd is not read.
template <bool PK, int IN = 6>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_policy_step_store_reset(const typename worker_policy::args_of<IN>::type pa, int n,
                                                                              float* __restrict__ st, float* __restrict__ obs_io,
                                                                              float* __restrict__ act_out, RingPtrs ring, int capacity,
                                                                              int next_idx, uint32_t k0, uint32_t k1, uint32_t c1,
                                                                              uint32_t c2, uint8_t* __restrict__ done_out, PreDraw pd) {
    if constexpr (IN == 6) {
        if (predraw_block<mlp::NTHREAD>(pd, ring, capacity, next_idx, n)) return;
    }
    __shared__ __attribute__((aligned(16))) float smem[worker_policy::smem_floats<IN>()];
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    __shared__ float sAct[mlp::GROUP * 2];
    worker_policy::group<PK, IN>(pa, n, obs_io, blockIdx.x, smem, sAct, act_out);
    group_env_lanes(n, worker_policy::obs_dim_of(pa), st, obs_io, sAct, s_quad, ring, capacity, next_idx, k0, k1, c1, c2, done_out);
}

// OffPolicyWorker.sample's inner body for a STOCHASTIC policy (worker.py:95-112 with the action sampled from the Gaussian head, no
// explore_sigma) in ONE launch: mpg_normal_fill + mpg_policy_sample (k_forward<IN, 4>, k_row_sums<HeadRow<PlainHead>>) + mpg_env_step_store_reset
// are four launches of at most one wave per CU each; here wave 0 draws and samples behind the four-logit pass
// (worker_policy::sample_group) and then steps the agents as in k_policy_step_store_reset.  No spare workgroups: there is no
// pre-gathered draw.  IN as in k_policy_step_store_reset.
template <bool PK, int IN>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_policy_sample_step_store_reset(const typename worker_policy::args_of<IN>::type pa,
                                                                                     int n, float* __restrict__ st,
                                                                                     float* __restrict__ obs_io, float* __restrict__ act_out,
                                                                                     float* __restrict__ logp_out, RingPtrs ring,
                                                                                     int capacity, int next_idx, uint32_t k0, uint32_t k1,
                                                                                     uint32_t c1, uint32_t c2,
                                                                                     uint8_t* __restrict__ done_out) {
    __shared__ __attribute__((aligned(16))) float smem[worker_policy::smem_floats<IN, 4>()];
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    __shared__ float sLogit[mlp::GROUP * 4];
    __shared__ float sAct[mlp::GROUP * 2];
    worker_policy::sample_group<PK, IN>(pa, n, obs_io, blockIdx.x, smem, sLogit, sAct, act_out, logp_out);
    group_env_lanes(n, worker_policy::obs_dim_of(pa), st, obs_io, sAct, s_quad, ring, capacity, next_idx, k0, k1, c1, c2, done_out);
}

// MPGLearner.sample / NDPGLearner.sample (mpg_learner.py:109-124, ndpg.py:99-114) in ONE launch: from obs0 take n real-env steps, the
// first with the replay action act0, the later ones with the policy's deterministic action.  The stand-alone chain is
// mpg_env_reset_from_obs + n x mpg_env_step + (n - 1) x mpg_policy_action = 2 n launches of one wave per CU each, every policy launch
// fetching the weights again.  Here the resident plan (policy_pass.h) on 16 rows for all n steps: wave 0 - four lanes per row,
// step_agent<4> - builds the agents from obs0 as k_reset_from_obs does; the policy is not evaluated at step 0.  Global memory is read
// in the prologue only (obs0, act0, weights) and written for rewards / last_obs only.  No done flag has a consumer (k_step does not
// reset, neither sample() nor mpg_nstep_targets reads them).  Rewards, last observations and the status word are bit-identical to the
// chain's: the same device functions on the same operands in the same order (tests/test_ndpg_gpu.py).  IN as in
// k_policy_step_store_reset.
template <bool PK, int IN>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_env_rollout(const typename worker_policy::args_of<IN>::type pa, int rows, int n,
                                                                  const float* __restrict__ obs0, const float* __restrict__ act0,
                                                                  float* __restrict__ rewards, float* __restrict__ last_obs) {
    __shared__ __attribute__((aligned(16))) float smem[worker_policy::smem_floats<IN>()];
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 16];
    __shared__ float sAct[mlp::GROUP * 2];
    const int od = worker_policy::obs_dim_of(pa);
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<IN, 2> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, IN, 2>(pa, 4, L, w2, r, b3v);
    // the env lanes: wave 0, four lanes per agent, each holding the whole agent (step_agent<4>)
    const int a_loc = threadIdx.x >> 2, q = threadIdx.x & 3, i = blockIdx.x * mlp::GROUP + a_loc;
    const bool env_lane_on = threadIdx.x < 64 && i < rows;
    Agent ag = {};
    float2 an = make_float2(0.f, 0.f);
    if (env_lane_on) {                                   // k_reset_from_obs: only the six base entries are read
        const float* o = obs0 + (size_t)i * od;
        const float dy = o[3], dphi = o[4];
        const PathRef p = path_ref(o[5]);
        ag.vx = o[0] + 20.f; ag.vy = o[1]; ag.r = o[2];
        ag.y = dy + p.y;
        ag.phi = dphi + p.phi;
        ag.x = o[5]; ag.dy = dy; ag.dphi = dphi;
        an = reinterpret_cast<const float2*>(act0)[i];
    }
    for (int t = 0; t < n; ++t) {
        if (t > 0) {
            mlp::lds_barrier();                          // sObs of step t - 1 is complete (and the previous pass's LDS is free)
            worker_policy::pass<IN, 2>(pa, rows, blockIdx.x, sObs, smem, sAct, L, w2, r, b3v, zmax, saw_nan);
            if (threadIdx.x < 64) {                      // wave 0 wrote sAct itself: LDS is in order within a wave
                __builtin_amdgcn_wave_barrier();
                an = make_float2(sAct[2 * a_loc], sAct[2 * a_loc + 1]);
            }
        }
        if (env_lane_on) {
            const StepOut o = step_agent<4>(ag, an, q, s_quad + a_loc * 100);
            if (q == 0) rewards[(size_t)t * rows + i] = o.reward;
            if (q == 1) {
                if (t == n - 1) write_obs(last_obs, i, od, ag);
                else write_obs(sObs, a_loc, od, ag);
            }
        }
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// ---- the resident kernels on the env's own state block: k_worker_rollout, k_worker_sample_rollout, k_eval_rollout ---------------------
// The resident plan of policy_pass.h with wave 0 as the env lanes, four lanes per agent, each holding the whole agent (step_agent<4>).
// State, obs_io, act_out and the done flags are written after the LAST iteration only: what the chain of launches leaves behind.

// Their prologue behind the policy's registers: the lane's agent (env lanes only), and the group's rows of obs_io (16 x od <= 256
// floats) into sObs.
__device__ __forceinline__ void resident_prologue(Agent& ag, int n, int od, int i_lane, const float* st, const float* obs_io, float* sObs) {
    if (threadIdx.x < 64 && i_lane < n) ag = load_agent(st, n, i_lane);
    const int g0 = blockIdx.x * mlp::GROUP, live = (n - g0 < mlp::GROUP ? n - g0 : mlp::GROUP) * od;
    if ((int)threadIdx.x < live) sObs[threadIdx.x] = obs_io[(size_t)g0 * od + threadIdx.x];
}

// What wave 0 needs of a worker rollout's arguments once per iteration.  They rest in LDS and are read where they are used: held in
// scalar registers for the whole loop, beside the env's hoisted constants, they and the Philox key schedules derived from them were
// spilled.  Head: what the policy's head adds - nothing, or the squashed Gaussian head's two constants.
struct NoHead {};
struct SquashHead {
    float range, log_r;            // SQ: the action range and its logarithm (gauss::log_range)
};
template <class Head>
struct RolloutEnvArgs {
    RingPtrs ring;
    float *st, *obs_io, *act_out;
    uint8_t* done_out;
    uint32_t k0, k1, pk0, pk1;     // env key, the policy's key (exploration noise or draw)
    uint64_t env_ctr, policy_ctr;  // the counters of iteration 0, carried as 64-bit sums
    uint32_t capacity;
    Head head;
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

// One iteration `it` of an env lane with its action in sAct: what env_lane<4> does, in its order - ring row (obs, act) at `slot`,
// step_agent<4>, (obs2, rew, done), reset_agent keyed (env key, env counter + it) if done, and the next observation: into sObs, or
// behind the last iteration state, obs_io and done_out - then the slot advanced by n (n <= capacity < 2^31: no overflow).
template <class A>
__device__ __forceinline__ void rollout_env_iteration(A& sArg, Agent& ag, uint32_t& slot, int it, bool last, int q, int i, int od, int n,
                                                      int a_loc, const float* sAct, float* sObs, float* s_quad) {
    if (i < n) {
        const float2 an = make_float2(sAct[2 * a_loc], sAct[2 * a_loc + 1]);
        if (q == 0) {
            write_obs(sArg.ring.obs, (int)slot, od, ag);             // obs before the step
            reinterpret_cast<float2*>(sArg.ring.act)[slot] = an;
        }
        const StepOut o = step_agent<4>(ag, an, q, s_quad + a_loc * 100);
        if (q == 1) {
            write_obs(sArg.ring.obs2, (int)slot, od, ag);
            sArg.ring.rew[slot] = o.reward;
            sArg.ring.done[slot] = o.done ? 1 : 0;
            uint8_t* const dn = sArg.done_out;
            if (last && dn) dn[i] = o.done ? 1 : 0;
        }
        if (o.done) {
            const uint64_t ec = sArg.env_ctr + (uint64_t)it;
            reset_agent(ag, i, sArg.k0, sArg.k1, (uint32_t)ec, (uint32_t)(ec >> 32));
        }
        if (last) {
            if (q == 2) store_agent(sArg.st, n, i, ag);
            if (q == 3) write_obs(sArg.obs_io, i, od, ag);
        } else if (q == 3) {
            write_obs(sObs, a_loc, od, ag);
        }
        slot += (uint32_t)n;
        if (slot >= sArg.capacity) slot -= sArg.capacity;
    }
}

// OffPolicyWorker.sample's `iters` iterations (worker.py:91-119: policy -> + N(0, sigma) -> env.step -> ring -> env.reset) in ONE
// launch: `iters` consecutive k_policy_step_store_reset launches with the noise and env counters and the ring position advancing by
// one / one / n per launch, each of which fetches the policy's weights and the agents' state again.  Between the pass and the env
// step lanes 0 .. 31 of wave 0 add the exploration noise (worker_policy::explore).  (noise / env) c1, c2: the counters of iteration 0.
// The host refuses iters * n > capacity: two iterations would write one ring slot from different workgroups.  Everything the chain
// leaves is bit-identical: the same device functions on the same operands in the same order (tests/test_worker_rollout_gpu.py).
// IN as in k_policy_step_store_reset.
template <bool PK, int IN>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_worker_rollout(const typename worker_policy::args_of<IN>::type pa, int n_launch,
                                                                     int iters, float* st, float* obs_io, float* act_out, RingPtrs ring, int capacity,
                                                                     int next_idx, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2,
                                                                     uint8_t* done_out) {
    __shared__ __attribute__((aligned(16))) float smem[worker_policy::smem_floats<IN>()];
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 16];
    __shared__ float sAct[mlp::GROUP * 2];
    __shared__ RolloutEnvArgs<NoHead> sArg;
    const int od_launch = worker_policy::obs_dim_of(pa);
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<IN, 2> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, IN, 2>(pa, 4, L, w2, r, b3v);
    const int a_loc = threadIdx.x >> 2, q_lane = threadIdx.x & 3, i_lane = blockIdx.x * mlp::GROUP + a_loc;
    Agent ag = {};
    resident_prologue(ag, n_launch, od_launch, i_lane, st, obs_io, sObs);
    if (threadIdx.x == 0) sArg.park(pa, st, obs_io, act_out, ring, capacity, k0, k1, c1, c2, done_out);
    // the agent's ring slot: (next_idx + it * n + i) % capacity
    uint32_t slot = (uint32_t)(((long)next_idx + i_lane) % capacity);
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        mlp::lds_barrier();                              // sObs of this iteration is complete (and the previous pass's LDS is free)
        worker_policy::pass<IN, 2>(pa, n_launch, blockIdx.x, sObs, smem, sAct, L, w2, r, b3v, zmax, saw_nan);
        if (threadIdx.x >= 64) continue;                 // wave 0 wrote sAct itself: LDS is in order within a wave
        // The lane's place and the launch's sizes, opaque per iteration: what is derived from them - the predicates q == 0 .. 3 and
        // i < n, row strides, the group's offset - is then formed where it is used and not held in scalar registers across the whole
        // loop beside the env's hoisted constants, which left no room for them (tools/kernel_resources.py: no spilled register)
        int q = q_lane, i = i_lane, od = od_launch, g = blockIdx.x, n = n_launch;
        asm volatile("" : "+v"(q), "+v"(i), "+s"(g), "+s"(n));
        if constexpr (IN == 16) asm volatile("" : "+s"(od));      // (a constant at IN = 6)
        if (threadIdx.x < mlp::GROUP * 2) {
            const uint64_t nc = sArg.policy_ctr + (uint64_t)it;
            const float y = worker_policy::explore(pa.sigma, n, g, sAct, sArg.pk0, sArg.pk1, (uint32_t)nc, (uint32_t)(nc >> 32), saw_nan);
            if (last && g * mlp::GROUP + (int)threadIdx.x / 2 < n) sArg.act_out[(size_t)g * mlp::GROUP * 2 + threadIdx.x] = y;
        }
        __builtin_amdgcn_wave_barrier();
        rollout_env_iteration(sArg, ag, slot, it, last, q, i, od, n, a_loc, sAct, sObs, s_quad);
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// The same `iters` iterations for a STOCHASTIC policy (SAC; worker.py:96: the action IS the sample, no explore_sigma): `iters`
// consecutive triples of mpg_normal_fill(2 n, sample key, sample counter + it), mpg_policy_sample (SQ: mpg_policy_sample_squashed -
// k_forward<IN, 4, PK, 1> and k_row_sums<HeadRow<PlainHead / SquashedHead>>) and mpg_env_step_store_reset in ONE launch; without SQ that is `iters`
// k_policy_sample_step_store_reset launches.  The policy's registers hold all four output columns.  Between the pass and the env step
// the four logits of a row lie in sLogit, left by the row's own four lanes; the first of them draws elements 2 i, 2 i + 1 of the
// iteration's stream, forms the action (worker_policy::sample_act) and leaves it in sAct for the four: LDS is in order within a wave.
// (pa.k0 .. pa.c2: the draw's key and the counter of iteration 0; pa.sigma, pa.out_scale: not read.)  IN as in
// k_policy_step_store_reset.
template <bool PK, int IN, bool SQ>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_worker_sample_rollout(const typename worker_policy::args_of<IN>::type pa, int n_launch,
                                                                            int iters, float* st, float* obs_io, float* act_out, RingPtrs ring,
                                                                            int capacity, int next_idx, uint32_t k0, uint32_t k1, uint32_t c1,
                                                                            uint32_t c2, uint8_t* done_out, float range, float log_r) {
    __shared__ __attribute__((aligned(16))) float smem[worker_policy::smem_floats<IN, 4>()];
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 16];
    __shared__ __attribute__((aligned(16))) float sLogit[mlp::GROUP * 4];
    __shared__ float sAct[mlp::GROUP * 2];
    __shared__ RolloutEnvArgs<SquashHead> sArg;
    const int od_launch = worker_policy::obs_dim_of(pa);
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<IN, 4> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, IN, 4>(pa, 4, L, w2, r, b3v);
    const int a_loc = threadIdx.x >> 2, q_lane = threadIdx.x & 3, i_lane = blockIdx.x * mlp::GROUP + a_loc;
    Agent ag = {};
    resident_prologue(ag, n_launch, od_launch, i_lane, st, obs_io, sObs);
    if (threadIdx.x == 0) {
        sArg.park(pa, st, obs_io, act_out, ring, capacity, k0, k1, c1, c2, done_out);
        sArg.head.range = range; sArg.head.log_r = log_r;
    }
    // the agent's ring slot: (next_idx + it * n + i) % capacity
    uint32_t slot = (uint32_t)(((long)next_idx + i_lane) % capacity);
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        mlp::lds_barrier();                              // sObs of this iteration is complete (and the previous pass's LDS is free)
        worker_policy::pass<IN, 4>(pa, n_launch, blockIdx.x, sObs, smem, sLogit, L, w2, r, b3v, zmax, saw_nan);
        if (threadIdx.x >= 64) continue;                 // wave 0 wrote sLogit itself: LDS is in order within a wave
        // (the lane's place and the launch's sizes, opaque per iteration: k_worker_rollout says why)
        int q = q_lane, i = i_lane, od = od_launch, n = n_launch;
        asm volatile("" : "+v"(q), "+v"(i), "+s"(n));
        if constexpr (IN == 16) asm volatile("" : "+s"(od));      // (a constant at IN = 6)
        __builtin_amdgcn_wave_barrier();
        if (i < n && q == 0) {                           // the first of the row's four lanes: the draw and the head
            const uint64_t sc = sArg.policy_ctr + (uint64_t)it;
            float act[2];
            worker_policy::sample_act<SQ>(sLogit + 4 * a_loc, i, sArg.head.range, sArg.head.log_r, sArg.pk0, sArg.pk1, (uint32_t)sc,
                                          (uint32_t)(sc >> 32), act);
            sAct[2 * a_loc] = act[0];
            sAct[2 * a_loc + 1] = act[1];
            if (last) {
                float* const ao = sArg.act_out + (size_t)i * 2;
                ao[0] = act[0];
                ao[1] = act[1];
            }
        }
        __builtin_amdgcn_wave_barrier();
        rollout_env_iteration(sArg, ag, slot, it, last, q, i, od, n, a_loc, sAct, sObs, s_quad);
    }
    policy_pass::report(pa, zmax, saw_nan);
}

// k_eval_rollout (below): what wave 0 needs of the launch's arguments once per step, resting in LDS as RolloutEnvArgs does and for its
// reason: seven pointers held in scalar registers across the whole loop, beside the env's hoisted constants, leave those no room.
struct EvalEnvArgs {
    float *st, *obs_io, *obs_traj, *act_traj, *rew_traj;
    uint8_t *done_out, *done_intended_out;
};

// Evaluator.run_n_episodes_parallel's loop (evaluator.py:132-139: compute_mode -> env.step, `done` not consulted, nothing reset) in ONE
// launch: `steps` consecutive pairs of mpg_policy_action (sigma 0) and mpg_env_step = 2 * steps launches of at most one wave per CU,
// every policy launch fetching the weights again and every env launch the state.  Unlike k_env_rollout the agents come from the env's
// own state block and the first observations from obs_io - a drawn state does not survive the round trip through its observation
// (reset_agent wraps phi, k_reset_from_obs does not) - the policy is evaluated at step 0 too, and the whole trajectory is recorded:
// per step t the observation BEFORE the step (out of sObs: at t = 0 the caller's own rows, later what write_obs left there) at
// obs_traj[(t n + i) od ..], the action as the pass formed it - unclipped, the env clips its own copy - at act_traj[(t n + i) 2 ..] and
// the reward at rew_traj[t n + i]: the layouts torch.stack gives the evaluator's per-step tensors.  The done flags are k_step's two,
// both nullable here.  Everything is bit-identical to the chain's: the same device functions on the same operands in the same order
// (tests/test_eval_rollout_gpu.py).  IN as in k_policy_step_store_reset.
// NO REGISTER HEADROOM: the packed IN = 6 form takes 254 of the 256 VGPRs this launch bound allows (strided 250; IN = 16: 238 / 235),
// without scratch.  A change to step_agent, worker_policy::pass, policy_pass::stage or this loop can tip it into scratch: run
// `tools/kernel_resources.py env_path_tracking.hip` after any such edit.
template <bool PK, int IN>
__global__ void __launch_bounds__(mlp::NTHREAD, 2) k_eval_rollout(const typename worker_policy::args_of<IN>::type pa, int n_launch,
                                                                   int steps, float* st, float* obs_io, float* obs_traj, float* act_traj,
                                                                   float* rew_traj, uint8_t* done_out, uint8_t* done_intended_out) {
    __shared__ __attribute__((aligned(16))) float smem[worker_policy::smem_floats<IN>()];
    __shared__ __attribute__((aligned(16))) float s_quad[16 * 100];
    __shared__ __attribute__((aligned(16))) float sObs[mlp::GROUP * 16];
    __shared__ float sAct[mlp::GROUP * 2];
    __shared__ EvalEnvArgs sArg;
    const int od_launch = worker_policy::obs_dim_of(pa);
    const mlp::Lane L;
    float w2[128];
    mlp::SmallRegs<IN, 2> r;
    float b3v, zmax = 0.f;
    bool saw_nan = false;
    policy_pass::load<PK, IN, 2>(pa, 4, L, w2, r, b3v);
    const int a_loc = threadIdx.x >> 2, q_lane = threadIdx.x & 3, i_lane = blockIdx.x * mlp::GROUP + a_loc;
    Agent ag = {};
    resident_prologue(ag, n_launch, od_launch, i_lane, st, obs_io, sObs);
    if (threadIdx.x == 0) {
        sArg.st = st; sArg.obs_io = obs_io; sArg.obs_traj = obs_traj; sArg.act_traj = act_traj; sArg.rew_traj = rew_traj;
        sArg.done_out = done_out; sArg.done_intended_out = done_intended_out;
    }
    for (int t = 0; t < steps; ++t) {
        const bool last = t == steps - 1;
        mlp::lds_barrier();                              // sObs of this step is complete (and the previous pass's LDS is free)
        worker_policy::pass<IN, 2>(pa, n_launch, blockIdx.x, sObs, smem, sAct, L, w2, r, b3v, zmax, saw_nan);
        if (threadIdx.x >= 64) continue;                 // wave 0 wrote sAct itself: LDS is in order within a wave
        // (the lane's place and the launch's sizes, opaque per step: k_worker_rollout says why)
        int q = q_lane, i = i_lane, od = od_launch, n = n_launch;
        asm volatile("" : "+v"(q), "+v"(i), "+s"(n));
        if constexpr (IN == 16) asm volatile("" : "+s"(od));      // (a constant at IN = 6)
        __builtin_amdgcn_wave_barrier();
        if (i < n) {
            const float2 an = make_float2(sAct[2 * a_loc], sAct[2 * a_loc + 1]);
            const size_t row = (size_t)t * (size_t)n + (size_t)i;
            {   // the observation before the step, lane q its entries q, q + 4, ..; the action by the first lane
                float* const ot = sArg.obs_traj + row * (size_t)od;
                for (int k = q; k < od; k += 4) ot[k] = sObs[a_loc * od + k];
                if (q == 0) reinterpret_cast<float2*>(sArg.act_traj)[row] = an;
            }
            const StepOut o = step_agent<4>(ag, an, q, s_quad + a_loc * 100);
            if (q == 1) {
                sArg.rew_traj[row] = o.reward;
                if (last) {
                    uint8_t* const dn = sArg.done_out;
                    uint8_t* const di = sArg.done_intended_out;
                    if (dn) dn[i] = o.done ? 1 : 0;
                    if (di) di[i] = o.done_intended ? 1 : 0;
                }
            }
            if (last) {
                if (q == 2) store_agent(sArg.st, n, i, ag);
                if (q == 3) write_obs(sArg.obs_io, i, od, ag);
            } else if (q == 3) {
                write_obs(sObs, a_loc, od, ag);
            }
        }
    }
    policy_pass::report(pa, zmax, saw_nan);
}

inline bool pt_obs_dim_ok(int od) { return od >= 6 && od <= 6 + MPG_ENV_MAX_FUTURE; }

}  // namespace

extern "C" int mpg_env_reset_from_obs(int env_kind, int n, int obs_dim, float* state, const float* init_obs, mpg_stream_t stream) {
    if (env_kind == MPG_ENV_INVERTED_PENDULUM) return cart_pole::reset_from_obs(n, obs_dim, state, init_obs, mpg_stream(stream));
    MPG_REQUIRE(env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "mpg_env_reset_from_obs: " MPG_NO_DOUBLE_PENDULUM_ENV);
    MPG_REQUIRE(env_kind == MPG_ENV_PATH_TRACKING, "mpg_env_reset_from_obs: unknown env kind %d", env_kind);
    MPG_REQUIRE(n > 0 && state && init_obs && pt_obs_dim_ok(obs_dim), "mpg_env_reset_from_obs: bad argument");
    hipLaunchKernelGGL(k_reset_from_obs, dim3((n + 63) / 64), dim3(64), 0, mpg_stream(stream), n, obs_dim, state, init_obs);
    MPG_CHECK_LAUNCH("mpg_env_reset_from_obs");
    return MPG_OK;
}

extern "C" int mpg_env_reset(int env_kind, int n, int obs_dim, float* state, const uint8_t* done_mask, uint64_t seed, uint64_t ctr,
                             float* obs, mpg_stream_t stream) {
    if (env_kind == MPG_ENV_INVERTED_PENDULUM) return cart_pole::reset(n, obs_dim, state, done_mask, seed, ctr, obs, mpg_stream(stream));
    MPG_REQUIRE(env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "mpg_env_reset: " MPG_NO_DOUBLE_PENDULUM_ENV);
    MPG_REQUIRE(env_kind == MPG_ENV_PATH_TRACKING, "mpg_env_reset: unknown env kind %d", env_kind);
    MPG_REQUIRE(n > 0 && state && obs && pt_obs_dim_ok(obs_dim), "mpg_env_reset: bad argument");
    hipLaunchKernelGGL(k_reset, dim3((n + 63) / 64), dim3(64), 0, mpg_stream(stream), n, state, done_mask, MPG_KEY_CTR(seed, ctr), obs,
                       obs_dim);
    MPG_CHECK_LAUNCH("mpg_env_reset");
    return MPG_OK;
}

extern "C" int mpg_env_step(int env_kind, int n, int obs_dim, float* state, const float* action, float* obs, float* reward,
                            uint8_t* done, uint8_t* done_intended, mpg_stream_t stream) {
    if (env_kind == MPG_ENV_INVERTED_PENDULUM)
        return cart_pole::step(n, obs_dim, state, action, obs, reward, done, done_intended, mpg_stream(stream));
    MPG_REQUIRE(env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "mpg_env_step: " MPG_NO_DOUBLE_PENDULUM_ENV);
    MPG_REQUIRE(env_kind == MPG_ENV_PATH_TRACKING, "mpg_env_step: unknown env kind %d", env_kind);
    MPG_REQUIRE(n > 0 && state && action && obs && reward && done && pt_obs_dim_ok(obs_dim), "mpg_env_step: bad argument");
    hipLaunchKernelGGL(k_step, dim3((n + 63) / 64), dim3(64), 0, mpg_stream(stream), n, state, action, obs, reward,
                       done, done_intended, obs_dim);
    MPG_CHECK_LAUNCH("mpg_env_step");
    return MPG_OK;
}

namespace {
// the caller's draw request as the kernels take it (pd.env_blocks is the launch's own); `who`: the entry point, for the refusal
int make_predraw(const char* who, const mpg_replay_draw_t* draw, int rows, float* b_obs, float* b_act, float* b_rew, float* b_obs2,
                 int capacity, PreDraw& pd) {
    MPG_REQUIRE(draw && rows > 0 && b_obs && b_act && b_rew && b_obs2 && draw->n_storage > 0 && draw->n_storage <= capacity,
                "%s: incomplete draw", who);
    pd.rows = rows; pd.n_storage = draw->n_storage;
    pd.k0 = (uint32_t)draw->seed; pd.k1 = (uint32_t)(draw->seed >> 32);
    pd.c1 = (uint32_t)draw->ctr; pd.c2 = (uint32_t)(draw->ctr >> 32);
    pd.o_idx = draw->idx_out; pd.o_done = draw->done_out;
    pd.o_obs = b_obs; pd.o_act = b_act; pd.o_rew = b_rew; pd.o_obs2 = b_obs2;
    return MPG_OK;
}

int step_store_reset_impl(int env_kind, int n, int obs_dim, float* state, const float* action, int capacity, int next_idx,
                          const RingPtrs& ring, uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out, PreDraw pd,
                          mpg_stream_t stream) {
    MPG_REQUIRE(ring_ok(n, capacity, next_idx, ring) && state && action && obs_out, "mpg_env_step_store_reset: bad argument");
    MPG_REQUIRE(env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "mpg_env_step_store_reset: " MPG_NO_DOUBLE_PENDULUM_ENV);
    if (env_kind == MPG_ENV_INVERTED_PENDULUM) {
        MPG_REQUIRE(pd.rows == 0, "mpg_env_step_store_reset_draw: path-tracking env only");
        return cart_pole::step_store_reset(n, obs_dim, state, action, capacity, next_idx, ring, seed, ctr, obs_out, done_out,
                                           mpg_stream(stream));
    }
    MPG_REQUIRE(env_kind == MPG_ENV_PATH_TRACKING, "mpg_env_step_store_reset: unknown env kind %d", env_kind);
    MPG_REQUIRE(pt_obs_dim_ok(obs_dim), "mpg_env_step_store_reset: obs_dim");
    // one lane per agent: the throughput form; four lanes per agent: the latency form
    const bool one_lane = n >= MPG_ENV_ONE_LANE_FROM;
    pd.env_blocks = ((one_lane ? 1 : 4) * n + 63) / 64;
    const int blocks = pd.env_blocks + (pd.rows + 63) / 64;
    hipLaunchKernelGGL(one_lane ? k_step_store_reset_1 : k_step_store_reset, dim3(blocks), dim3(64), 0, mpg_stream(stream), n, state,
                       action, ring, capacity, next_idx, MPG_KEY_CTR(seed, ctr), obs_out, done_out, obs_dim, pd);
#ifdef MPG_TIMELINE
    static int s_calls = 0;
    if (!one_lane && ++s_calls % 100 == 0) {
        unsigned long long h[2][16];
        (void)hipStreamSynchronize(mpg_stream(stream));
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_env_tl), sizeof(h));
        for (int b = 0; b < 2; ++b) {
            fprintf(stderr, "timeline env wg%d:", b ? 200 : 0);
            for (int k = 1; k < 9; ++k) fprintf(stderr, " %d:%lld", k, (long long)(h[b][k] - h[b][0]));
            fprintf(stderr, "\n");
        }
    }
#endif
    MPG_CHECK_LAUNCH("mpg_env_step_store_reset");
    return MPG_OK;
}
}  // namespace

extern "C" int mpg_env_step_store_reset(int env_kind, int n, int obs_dim, float* state, const float* action, int capacity, int next_idx,
                                        float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                                        uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out, mpg_stream_t stream) {
    return step_store_reset_impl(env_kind, n, obs_dim, state, action, capacity, next_idx,
                                 RingPtrs{ring_obs, ring_act, ring_rew, ring_obs2, ring_done}, seed, ctr, obs_out, done_out, PreDraw{}, stream);
}

extern "C" int mpg_env_step_store_reset_draw(int env_kind, int n, int obs_dim, float* state, const float* action, int capacity,
                                             int next_idx, float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2,
                                             uint8_t* ring_done, uint64_t seed, uint64_t ctr, float* obs_out, uint8_t* done_out,
                                             const mpg_replay_draw_t* draw, int rows, float* b_obs, float* b_act, float* b_rew,
                                             float* b_obs2, mpg_stream_t stream) {
    MPG_REQUIRE(env_kind == MPG_ENV_PATH_TRACKING && obs_dim == 6, "mpg_env_step_store_reset_draw: path-tracking env with obs_dim 6 only");
    PreDraw pd{};
    if (int rc = make_predraw("mpg_env_step_store_reset_draw", draw, rows, b_obs, b_act, b_rew, b_obs2, capacity, pd)) return rc;
    return step_store_reset_impl(env_kind, n, obs_dim, state, action, capacity, next_idx,
                                 RingPtrs{ring_obs, ring_act, ring_rew, ring_obs2, ring_done}, seed, ctr, obs_out, done_out, pd, stream);
}

// worker.py:95-112 for the path-tracking env: mpg_policy_action + mpg_env_step_store_reset(_draw) as one launch (bit-identical actions,
// ring rows, states and observations).  obs_io [n][obs_dim]: the current observations in, the next ones out.  obs_dim 6 .. 16; the
// pre-gathered draw with six-entry observations only.
namespace {
template <class A>
void fill_policy_args(A& pa, int n_scale, const mpg_cfg_t* cfg, const float* policy_params, float explore_sigma, uint64_t noise_seed,
                      uint64_t noise_ctr) {
    pa.params = policy_params;
    pa.pack = mlp::weight_cache_lookup(cfg, mlp::make_net(policy_params, cfg->obs_dim, 4).W2, 0);
    pa.status = mpg_status_of(cfg);
    const bool ranged = cfg->action_range > 0.f;
    pa.out_tanh = (cfg->policy_out_act == MPG_ACT_TANH || ranged) ? 1 : 0;
    pa.out_scale = ranged ? cfg->action_range : 1.f;
    pa.sigma = explore_sigma;
    pa.k0 = (uint32_t)noise_seed; pa.k1 = (uint32_t)(noise_seed >> 32); pa.c1 = (uint32_t)noise_ctr; pa.c2 = (uint32_t)(noise_ctr >> 32);
    for (int i = 0; i < n_scale; ++i) pa.scale[i] = i < cfg->obs_dim ? cfg->obs_scale[i] : 1.f;
}

// The policy arguments of a launch and the instantiation that takes them: Args for six-entry observations, WideArgs beyond; packed when
// the weight cache holds W2's image.  launch(std::bool_constant<PK>, std::integral_constant<int, IN>, pa) issues the entry point's kernel.
template <class Launch>
void with_policy_args(const mpg_cfg_t* cfg, const float* policy_params, float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr,
                      Launch&& launch) {
    if (cfg->obs_dim > 6) {
        worker_policy::WideArgs pa;
        fill_policy_args(pa, 16, cfg, policy_params, explore_sigma, noise_seed, noise_ctr);
        pa.obs_dim = cfg->obs_dim;
        if (pa.pack) launch(std::true_type{}, std::integral_constant<int, 16>{}, pa);
        else launch(std::false_type{}, std::integral_constant<int, 16>{}, pa);
    } else {
        worker_policy::Args pa;
        fill_policy_args(pa, 8, cfg, policy_params, explore_sigma, noise_seed, noise_ctr);
        if (pa.pack) launch(std::true_type{}, std::integral_constant<int, 6>{}, pa);
        else launch(std::false_type{}, std::integral_constant<int, 6>{}, pa);
    }
}
}  // namespace

extern "C" int mpg_worker_step(const mpg_cfg_t* cfg, const float* policy_params, int n, float* state, float* obs_io, float explore_sigma,
                               uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity, int next_idx, float* ring_obs,
                               float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done, uint64_t env_seed,
                               uint64_t env_ctr, uint8_t* done_out, const mpg_replay_draw_t* draw, int rows, float* b_obs, float* b_act,
                               float* b_rew, float* b_obs2, mpg_stream_t stream) {
    MPG_REQUIRE(!cfg || cfg->env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "mpg_worker_step: " MPG_NO_DOUBLE_PENDULUM_ENV);
    MPG_REQUIRE(cfg && cfg->env_kind == MPG_ENV_PATH_TRACKING && pt_obs_dim_ok(cfg->obs_dim) && cfg->act_dim == 2,
                "mpg_worker_step: path-tracking env with obs_dim 6 .. 16 only");
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    MPG_REQUIRE(policy_params && ring_ok(n, capacity, next_idx, ring) && state && obs_io && act_out, "mpg_worker_step: bad argument");
    if (int rc = tanh_range_refusal("mpg_worker_step", cfg)) return rc;
    const bool wide = cfg->obs_dim > 6;
    // the rows are gathered six wide (predraw_row) for the fused gradient launch, which exists for six-entry observations only
    MPG_REQUIRE(!(draw && wide), "mpg_worker_step: the pre-gathered draw serves obs_dim 6 only (got obs_dim %d: pass draw = NULL)", cfg->obs_dim);
    PreDraw pd{};
    if (draw)
        if (int rc = make_predraw("mpg_worker_step", draw, rows, b_obs, b_act, b_rew, b_obs2, capacity, pd)) return rc;
    pd.env_blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    const int blocks = pd.env_blocks + (pd.rows + mlp::NTHREAD - 1) / mlp::NTHREAD;
    hipStream_t s = mpg_stream(stream);
    // (wide: pd.rows == 0, the grid is the policy groups)
    with_policy_args(cfg, policy_params, explore_sigma, noise_seed, noise_ctr, [&](auto pk, auto in, const auto& pa) {
        mpg_prof_begin(mpg_prof_of(cfg), 2, s);
        hipLaunchKernelGGL((k_policy_step_store_reset<decltype(pk)::value, decltype(in)::value>), dim3(blocks), dim3(mlp::NTHREAD), 0, s,
                           pa, n, state, obs_io, act_out, ring, capacity, next_idx, MPG_KEY_CTR(env_seed, env_ctr), done_out, pd);
    });
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_step");
    return MPG_OK;
}

// worker.py:91-119 for the path-tracking env: `iters` consecutive mpg_worker_step calls (draw = NULL; noise_ctr + it, ring position
// (next_idx + it * n) % capacity, env_ctr + it) as one launch (k_worker_rollout: bit-identical state, observations, actions, done
// flags, ring arrays and status word)
extern "C" int mpg_worker_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                                  float explore_sigma, uint64_t noise_seed, uint64_t noise_ctr, float* act_out, int capacity, int next_idx,
                                  float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done, uint64_t env_seed,
                                  uint64_t env_ctr, uint8_t* done_out, mpg_stream_t stream) {
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    if (int rc = env_cfg_refusal("mpg_worker_rollout", PATH_TRACKING_ENV, cfg)) return rc;
    if (int rc = tanh_range_refusal("mpg_worker_rollout", cfg)) return rc;
    if (int rc = ring_rollout_refusal("mpg_worker_rollout", policy_params && state && obs_io && act_out, n, iters, capacity, next_idx, ring))
        return rc;
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args(cfg, policy_params, explore_sigma, noise_seed, noise_ctr, [&](auto pk, auto in, const auto& pa) {
        mpg_prof_begin(mpg_prof_of(cfg), 2, s);
        hipLaunchKernelGGL((k_worker_rollout<decltype(pk)::value, decltype(in)::value>), dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, n,
                           iters, state, obs_io, act_out, ring, capacity, next_idx, MPG_KEY_CTR(env_seed, env_ctr), done_out);
    });
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_rollout");
    return MPG_OK;
}

// worker.py:68-79 (stochastic policy, explore_sigma unset) for the path-tracking env: mpg_normal_fill(2 n, sample_seed, sample_ctr) +
// mpg_policy_sample + mpg_env_step_store_reset as one launch (bit-identical actions, log-densities, ring rows, states, observations,
// done flags and status word)
extern "C" int mpg_worker_sample_step(const mpg_cfg_t* cfg, const float* policy_params, int n, float* state, float* obs_io,
                                      uint64_t sample_seed, uint64_t sample_ctr, float* act_out, float* logp_out, int capacity, int next_idx,
                                      float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                                      uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out, mpg_stream_t stream) {
    MPG_REQUIRE(!cfg || cfg->env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "mpg_worker_sample_step: " MPG_NO_DOUBLE_PENDULUM_ENV);
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    // what mpg_policy_sample refuses (its logp_out may be null here), then what mpg_worker_step asks of the ring
    if (int rc = gauss::gauss_refusal("mpg_worker_sample_step", cfg, policy_params && state && obs_io && act_out && ring.obs &&
                                           ring.act && ring.rew && ring.obs2 && ring.done, n, 0.f))
        return rc;
    MPG_REQUIRE(ring_ok(n, capacity, next_idx, ring), "mpg_worker_sample_step: bad ring (capacity %d < n %d, or next_idx %d outside it)",
                capacity, n, next_idx);
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args(cfg, policy_params, 0.f, sample_seed, sample_ctr, [&](auto pk, auto in, const auto& pa) {
        mpg_prof_begin(mpg_prof_of(cfg), 2, s);
        hipLaunchKernelGGL((k_policy_sample_step_store_reset<decltype(pk)::value, decltype(in)::value>), dim3(blocks), dim3(mlp::NTHREAD),
                           0, s, pa, n, state, obs_io, act_out, logp_out, ring, capacity, next_idx, MPG_KEY_CTR(env_seed, env_ctr),
                           done_out);
    });
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_sample_step");
    return MPG_OK;
}

// mpg_learner.py:109-124 / ndpg.py:99-114 for the path-tracking env: mpg_env_reset_from_obs + n x (mpg_policy_action from the second
// step on, mpg_env_step) as one launch (k_env_rollout: bit-identical rewards, last observations and status word).
extern "C" int mpg_env_rollout(const mpg_cfg_t* cfg, const float* policy_params, int rows, int n, const float* obs0, const float* act0,
                               float* rewards, float* last_obs, mpg_stream_t stream) {
    if (int rc = env_cfg_refusal("mpg_env_rollout", PATH_TRACKING_ENV, cfg)) return rc;
    MPG_REQUIRE(n >= 1 && n < 32, "mpg_env_rollout: 1 <= n < 32 steps (got %d)", n);
    MPG_REQUIRE(rows > 0, "mpg_env_rollout: no rows");
    MPG_REQUIRE(policy_params && obs0 && act0 && rewards && last_obs, "mpg_env_rollout: null pointer");
    if (int rc = tanh_range_refusal("mpg_env_rollout", cfg)) return rc;
    const int blocks = (rows + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args(cfg, policy_params, 0.f, 0, 0, [&](auto pk, auto in, const auto& pa) {
        hipLaunchKernelGGL((k_env_rollout<decltype(pk)::value, decltype(in)::value>), dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, rows, n,
                           obs0, act0, rewards, last_obs);
    });
    MPG_CHECK_LAUNCH("mpg_env_rollout");
    return MPG_OK;
}

// worker.py:91-119 for the path-tracking env under a stochastic policy: `iters` consecutive triples mpg_normal_fill(2 n, sample_seed,
// sample_ctr + it) + mpg_policy_sample (with cfg->action_range > 0: mpg_policy_sample_squashed) + mpg_env_step_store_reset (ring position
// (next_idx + it * n) % capacity, env_ctr + it) as one launch (k_worker_sample_rollout: bit-identical state, observations, actions, done
// flags, ring arrays and status word)
extern "C" int mpg_worker_sample_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int iters, float* state, float* obs_io,
                                         uint64_t sample_seed, uint64_t sample_ctr, float* act_out, int capacity, int next_idx,
                                         float* ring_obs, float* ring_act, float* ring_rew, float* ring_obs2, uint8_t* ring_done,
                                         uint64_t env_seed, uint64_t env_ctr, uint8_t* done_out, mpg_stream_t stream) {
    const RingPtrs ring{ring_obs, ring_act, ring_rew, ring_obs2, ring_done};
    if (int rc = env_cfg_refusal("mpg_worker_sample_rollout", PATH_TRACKING_ENV, cfg)) return rc;
    // no action range: the Gaussian head as it stands; a range: the squashed head, and what it asks of a cfg (a linear output, a finite
    // range; the pointers and the row count are judged below, with the ring)
    const bool squash = cfg->action_range > 0.f;
    if (squash)
        if (int rc = gauss::squash_refusal("mpg_worker_sample_rollout", cfg, true, 1, 0.f)) return rc;
    if (int rc = ring_rollout_refusal("mpg_worker_sample_rollout", policy_params && state && obs_io && act_out, n, iters, capacity, next_idx,
                                      ring))
        return rc;
    const float range = squash ? cfg->action_range : 0.f, log_r = squash ? gauss::log_range(cfg->action_range) : 0.f;
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args(cfg, policy_params, 0.f, sample_seed, sample_ctr, [&](auto pk, auto in, auto pa) {
        pa.out_tanh = cfg->policy_out_act == MPG_ACT_TANH;      // the logits' activation (logits_out): an action range never reaches them
        mpg_prof_begin(mpg_prof_of(cfg), 2, s);
        auto launch = [&](auto sq) {
            hipLaunchKernelGGL((k_worker_sample_rollout<decltype(pk)::value, decltype(in)::value, decltype(sq)::value>), dim3(blocks),
                               dim3(mlp::NTHREAD), 0, s, pa, n, iters, state, obs_io, act_out, ring, capacity, next_idx,
                               MPG_KEY_CTR(env_seed, env_ctr), done_out, range, log_r);
        };
        if (squash) launch(std::true_type{}); else launch(std::false_type{});
    });
    mpg_prof_end(mpg_prof_of(cfg), 2, s);
    MPG_CHECK_LAUNCH("mpg_worker_sample_rollout");
    return MPG_OK;
}

// evaluator.py:132-139 for the path-tracking env: `steps` consecutive pairs mpg_policy_action (explore_sigma 0) + mpg_env_step as one
// launch (k_eval_rollout: bit-identical trajectories, state, observations, done flags and status word)
extern "C" int mpg_eval_rollout(const mpg_cfg_t* cfg, const float* policy_params, int n, int steps, float* state, float* obs_io,
                                float* obs_traj, float* act_traj, float* rew_traj, uint8_t* done_out, uint8_t* done_intended_out,
                                mpg_stream_t stream) {
    if (int rc = env_cfg_refusal("mpg_eval_rollout", PATH_TRACKING_ENV, cfg)) return rc;
    if (int rc = eval_rollout_refusal("mpg_eval_rollout", n, steps, policy_params && state && obs_io && obs_traj && act_traj && rew_traj))
        return rc;
    if (int rc = tanh_range_refusal("mpg_eval_rollout", cfg)) return rc;
    const int blocks = (n + mlp::GROUP - 1) / mlp::GROUP;
    hipStream_t s = mpg_stream(stream);
    with_policy_args(cfg, policy_params, 0.f, 0, 0, [&](auto pk, auto in, const auto& pa) {
        hipLaunchKernelGGL((k_eval_rollout<decltype(pk)::value, decltype(in)::value>), dim3(blocks), dim3(mlp::NTHREAD), 0, s, pa, n, steps,
                           state, obs_io, obs_traj, act_traj, rew_traj, done_out, done_intended_out);
    });
    MPG_CHECK_LAUNCH("mpg_eval_rollout");
    return MPG_OK;
}

// ---- mpg_mpc_rollout: the MPC side of the closed loop of mpc/main.py:168-223 in one launch --------------------------------------------
namespace {

// `steps` times: record the observation, solve from it (mpc::solve, the body of k_mpc_solve in mpc_kernels.hip), record the plan, step
// the env with the plan's first pair (step_agent<1>, the body of k_step).  One lane per agent, workgroups of one wave: the agent's
// state block and its observation stay in registers across the steps, the solver's four arrays in dynamic LDS as in k_mpc_solve.
// What the chain of launches hands on through global memory is handed on here in registers and LDS, the same float32 values:
//   the observation: write_obs's entries (v_x - 20 first), to which the next step's start state adds (20, 0, 0, 0, 0, 0) as run_mpc's
//     obs + shift does - entry 0 is (v_x - 20) + 20, NOT v_x, and the sum with 0 turns a -0 into +0;
//   the start point: warm, the solution moved up by one pair inside U (k_mpc_solve would clamp what it reads, which leaves entries of
//     the box, NaN and -0 included, as they are); cold, u_io again - the one array read after the prologue, and one this kernel never
//     writes in that mode.
// State, obs_io, the done flags and (warm) u_io are written after the LAST step only.  Every loop has a fixed bound and leaves early
// only on a wave-uniform condition (mpc::solve says how); lanes behind the last agent solve nothing, step nothing and store nothing.
// The launch's pointers but u_io, the agent count, the warm-start flag and the tolerance rest in LDS, as EvalEnvArgs does for
// k_eval_rollout and for its reason: held in scalar registers across the solver's nested loops, beside the constants of the model and
// of the env that the compiler hoists out of the step loop, they spilled 25 of them (tools/kernel_resources.py); with only the pointers
// moved, two.  What comes back out of LDS is a vector register: the tolerance is only ever compared with a lane's own norm.
struct MpcRolloutArgs {
    float *st, *obs_io, *obs_traj, *plan_traj, *rew_traj, *cost_traj, *pgnorm_traj;
    int* info_traj;
    uint8_t *done_out, *done_intended_out;
    int n, warm;
    float tol;
};
__global__ void __launch_bounds__(mpc::WAVE) k_mpc_rollout(const MpcRolloutArgs a, int steps, int H, int iters, float* u_io) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ MpcRolloutArgs sArg;
    constexpr int W = mpc::WAVE;
    const int lane = threadIdx.x, i = blockIdx.x * W + lane;
    const bool valid = i < a.n;
    if (lane == 0) sArg = a;                    // (one wave: LDS is in order within it)
    float* U = lds + lane;                      // the last accepted point [2 H][W]; between two solves the next one's start point
    float* G = U + 2 * H * W;                   // its gradient
    float* T = G + 2 * H * W;                   // the trial point
    float* X = T + 2 * H * W;                   // the states of the last forward pass [NX H][W]
    Agent ag = {};
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, o4 = 0.f, o5 = 0.f;      // the observation (an idle lane's gives mpc::idle_state())
    float* const start = u_io + (size_t)(valid ? i : 0) * 2 * H;      // this lane's row of u_io, kept as the lane's own pointer
    if (valid) {
        ag = load_agent(a.st, a.n, i);
        const float* o = a.obs_io + (size_t)i * 6;
        o0 = o[0]; o1 = o[1]; o2 = o[2]; o3 = o[3]; o4 = o[4]; o5 = o[5];
    }
    // (the copy loops here are kept rolled: unrolled, their precomputed trip counts were what the step loop had no scalar register for)
#pragma unroll 1
    for (int j = 0; j < 2 * H; ++j) U[j * W] = valid ? mpc::box(start[j]) : 0.f;
    StepOut so = {};
    size_t row = (size_t)i;                     // t n + i
    __builtin_amdgcn_wave_barrier();
    const float tol = sArg.tol;
    for (int left = steps; left > 0; --left) {
        if (valid) {
            float* ot = sArg.obs_traj + row * 6;
            ot[0] = o0; ot[1] = o1; ot[2] = o2; ot[3] = o3; ot[4] = o4; ot[5] = o5;
        }
        const mpc::State s0 = {o0 + 20.f, o1 + 0.f, o2 + 0.f, o3 + 0.f, o4 + 0.f, o5 + 0.f};
        const mpc::Solved r = mpc::solve(H, iters, tol, valid, s0, U, G, T, X);
        const float2 an = make_float2(U[0], U[W]);
        if (valid) {
            float* pt = sArg.plan_traj + row * 2 * H;
#pragma unroll 1
            for (int j = 0; j < 2 * H; ++j) pt[j] = U[j * W];
            float* const ct = sArg.cost_traj;
            float* const gt = sArg.pgnorm_traj;
            int* const it = sArg.info_traj;
            if (ct) ct[row] = r.cost;
            if (gt) gt[row] = r.pgnorm;
            if (it) it[row] = r.info;
        }
        // the next solve's start point (behind the last step: what u_io takes, or nothing)
        if (__builtin_amdgcn_readfirstlane(sArg.warm)) {      // main.py:214: the plan one step later, its last pair repeated
#pragma unroll 1
            for (int j = 0; j + 2 < 2 * H; ++j) U[j * W] = U[(j + 2) * W];
        } else {                                               // :184: the caller's, which this launch never writes
#pragma unroll 1
            for (int j = 0; j < 2 * H; ++j) U[j * W] = valid ? mpc::box(start[j]) : 0.f;
        }
        if (valid) {
            so = step_agent<1>(ag, an);
            sArg.rew_traj[row] = so.reward;
            o0 = ag.vx - 20.f; o1 = ag.vy; o2 = ag.r; o3 = ag.dy; o4 = ag.dphi; o5 = ag.x;      // write_obs
        }
        row += (size_t)sArg.n;
    }
    if (valid) {
        store_agent(sArg.st, sArg.n, i, ag);
        write_obs(sArg.obs_io, i, 6, ag);
        uint8_t* const dn = sArg.done_out;
        uint8_t* const di = sArg.done_intended_out;
        if (dn) dn[i] = so.done ? 1 : 0;
        if (di) di[i] = so.done_intended ? 1 : 0;
        if (sArg.warm) {
#pragma unroll 1
            for (int j = 0; j < 2 * H; ++j) start[j] = U[j * W];
        }
    }
}

}  // namespace

extern "C" int mpg_mpc_rollout(int n, int steps, int horizon, int iters, float tol, int warm_start, float* state, float* obs_io, float* u_io,
                               float* obs_traj, float* plan_traj, float* rew_traj, float* cost_traj, float* pgnorm_traj, int* info_traj,
                               uint8_t* done_out, uint8_t* done_intended_out, mpg_stream_t stream) {
    MPG_REQUIRE(n > 0, "mpg_mpc_rollout: no agents (n %d)", n);
    MPG_REQUIRE(steps >= 1, "mpg_mpc_rollout: steps >= 1 (got %d)", steps);
    MPG_REQUIRE(steps <= MPG_MPC_ROLLOUT_MAX_STEPS, "mpg_mpc_rollout: steps <= %d (got %d)", MPG_MPC_ROLLOUT_MAX_STEPS, steps);
    MPG_REQUIRE(horizon >= 1, "mpg_mpc_rollout: horizon >= 1 (got %d)", horizon);
    MPG_REQUIRE(horizon <= MPG_MPC_MAX_HORIZON, "mpg_mpc_rollout: horizon <= %d (got %d)", MPG_MPC_MAX_HORIZON, horizon);
    MPG_REQUIRE(iters >= 0, "mpg_mpc_rollout: iters >= 0 (got %d)", iters);
    MPG_REQUIRE(iters <= MPG_MPC_MAX_ITERS, "mpg_mpc_rollout: iters <= %d (got %d)", MPG_MPC_MAX_ITERS, iters);
    // (one launch's run time on a shared device: include/mpg_hip.h derives the bound; callers run longer loops in chunks)
    MPG_REQUIRE((long)steps * iters <= MPG_MPC_ROLLOUT_MAX_WORK, "mpg_mpc_rollout: steps * iters = %ld solver iterations in one launch, at most %d",
                (long)steps * iters, MPG_MPC_ROLLOUT_MAX_WORK);
    MPG_REQUIRE(tol >= 0.f, "mpg_mpc_rollout: tol negative or NaN (%g)", (double)tol);
    MPG_REQUIRE(warm_start == 0 || warm_start == 1, "mpg_mpc_rollout: warm_start is 0 or 1 (got %d)", warm_start);
    MPG_REQUIRE(state && obs_io && u_io && obs_traj && plan_traj && rew_traj, "mpg_mpc_rollout: null pointer");
    const size_t lds = mpc::lds_bytes(horizon, 3);
    if (int rc = mpc::allow_lds("mpg_mpc_rollout", k_mpc_rollout, lds)) return rc;
    const MpcRolloutArgs a = {state, obs_io, obs_traj, plan_traj, rew_traj, cost_traj, pgnorm_traj, info_traj, done_out, done_intended_out,
                              n, warm_start, tol};
    hipLaunchKernelGGL(k_mpc_rollout, dim3((n + mpc::WAVE - 1) / mpc::WAVE), dim3(mpc::WAVE), lds, mpg_stream(stream), a, steps, horizon, iters,
                       u_io);
    MPG_CHECK_LAUNCH("mpg_mpc_rollout");
    return MPG_OK;
}
