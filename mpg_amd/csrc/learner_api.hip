// C-ABI entry points built from the generic network kernels: policy actions, critic targets, critic loss +
// gradient.  (The fused n-step rollout lives in rollout_kernels.hip, the optimizer in optim_kernels.hip.)
#include "gauss_head.h"
#include "host_glue.h"

using namespace mlp;
using namespace gauss;

namespace {

// y = (rew + shift) * scale + gamma * min(q1, q2)      (q2 == nullptr: q1 only)
__global__ void k_combine_target(int n, const float* __restrict__ rew, const float* __restrict__ q1,
                                 const float* __restrict__ q2, float shift, float scale, float gamma,
                                 float* __restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float q = q2 ? fminf(q1[i], q2[i]) : q1[i];
    y[i] = (rew[i] + shift) * scale + gamma * q;
}

// a += clip(sigma * eps, -c, c)      (td3.py:74-76)
__global__ void k_smooth(int n, float* __restrict__ a, const float* __restrict__ eps, float sigma, float c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a[i] += fminf(fmaxf(sigma * eps[i], -c), c);
}

// the two above in one launch (mpg_td3_targets: the plain Q1 target of the priorities, then the smoothing of the action for the
// clipped double-Q target - two dependent ~5 us launches at any batch size)
__global__ void k_combine_and_smooth(int rows, int ad, const float* __restrict__ rew, const float* __restrict__ q1, float shift, float scale,
                                     float gamma, float* __restrict__ y1, float* __restrict__ a, const float* __restrict__ eps, float sigma,
                                     float c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) y1[i] = (rew[i] + shift) * scale + gamma * q1[i];
    if (i < rows * ad) a[i] += fminf(fmaxf(sigma * eps[i], -c), c);
}

// y = sum_t gamma^t (r_t + shift) * scale + gamma^n q          (mpg_learner.py:165-168)
__global__ void k_nstep(int rows, int n, const float* __restrict__ rewards, const float* __restrict__ q, float shift,
                        float scale, float gamma, float* __restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    float acc = 0.f;
    for (int t = 0; t < n; ++t) acc += powf(gamma, (float)t) * ((rewards[(size_t)t * rows + i] + shift) * scale);
    y[i] = acc + powf(gamma, (float)n) * q[i];
}

// the same with the bootstrap value clipped to [lo, hi] first (the pendulum's target, mpg_learner.py:163-164: tf.clip_by_value =
// minimum(maximum(q, lo), hi), which hands a NaN on - fmaxf / fminf would return the bound - so the comparisons are written out).
// A kernel of its own: as one template over the clip, whichever of the two reads q[i] at the other's place in the statement order
// loses its instructions (EXPERIMENTS.md, "One policy head and one temperature type").
__global__ void k_nstep_clipped(int rows, int n, const float* __restrict__ rewards, const float* __restrict__ q, float shift,
                                float scale, float gamma, float lo, float hi, float* __restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    float acc = 0.f;
    for (int t = 0; t < n; ++t) acc += powf(gamma, (float)t) * ((rewards[(size_t)t * rows + i] + shift) * scale);
    float qv = q[i];
    qv = qv < lo ? lo : qv;          // a NaN compares false both times and stays
    qv = qv > hi ? hi : qv;
    y[i] = acc + powf(gamma, (float)n) * qv;
}

// ---- row sums: the element-wise pass of a loss over the rows of a batch together with the one or two sums it reports ----------------
// A row body carries its pointers and scalars, NS (the number of sums), SUM_OPTIONAL (whether a null destination means "no sum
// wanted"), scale0() (what the finished first sum is multiplied by; the second is reported as it is) and operator()(i, s): the stores
// of row i and its terms added into s[NS].
constexpr int ERR_PARTS = 64;
constexpr int ERR_MB_MIN_ROWS = 8192;          // below: the one-block form (one launch instead of two)
// a row body may also carry scale1(), what its finished SECOND sum is multiplied by (HeadRow2); without one it is reported as it is
template <class Row, class = void>
struct Scale1 {
    static constexpr bool ANY = false;
    static float of(const Row&) { return 1.f; }
};
template <class Row>
struct Scale1<Row, decltype((void)&Row::scale1)> {
    static constexpr bool ANY = true;
    static float of(const Row& r) { return r.scale1(); }
};

// critic loss: err = q - y; dz3 = err * inv_b; td (nullable) = err; the sum of err^2, finished as the loss 0.5 * inv_b * sum
struct QErrRow {
    const float *__restrict__ q, *__restrict__ y;
    float inv_b;
    float *__restrict__ dz3, *__restrict__ td;
    static constexpr int NS = 1;
    static constexpr bool SUM_OPTIONAL = false;
    __host__ __device__ float scale0() const { return 0.5f * inv_b; }
    __device__ __forceinline__ void operator()(int i, float* s) const {
        const float e = q[i] - y[i];
        dz3[i] = e * inv_b;
        if (td) td[i] = e;
        s[0] += e * e;
    }
};
// TD3 policy loss pieces (td3.py:120-134): qmin = min(q1, q2); dL/dq_i = -inv_b where q_i is the smaller one (tf.reduce_min routes
// the gradient to the minimum; exact ties go to Q1); the sums of qmin and qmin^2 (value_mean / value_var)
struct Td3DyRow {
    const float *__restrict__ q1, *__restrict__ q2;
    float inv_b;
    float *__restrict__ dy1, *__restrict__ dy2;
    static constexpr int NS = 2;
    static constexpr bool SUM_OPTIONAL = false;
    __host__ __device__ float scale0() const { return 1.f; }
    __device__ __forceinline__ void operator()(int i, float* s) const {
        const bool first = q1[i] <= q2[i];
        const float m = first ? q1[i] : q2[i];
        dy1[i] = first ? -inv_b : 0.f;
        dy2[i] = first ? 0.f : -inv_b;
        s[0] += m;
        s[1] += m * m;
    }
};
// n-step DPG policy loss pieces (ndpg.py:174-186): one critic, so dL/dq = -inv_b for every row; the sums of q and q^2
struct DpgDyRow {
    const float* __restrict__ q;
    float inv_b;
    float* __restrict__ dy;
    static constexpr int NS = 2;
    static constexpr bool SUM_OPTIONAL = false;
    __host__ __device__ float scale0() const { return 1.f; }
    __device__ __forceinline__ void operator()(int i, float* s) const {
        const float m = q[i];
        dy[i] = -inv_b;
        s[0] += m;
        s[1] += m * m;
    }
};

// Thread t of a block walks the rows t, t + 1024, ... of the block's run; a 1024-wide tree (512 -> 1) adds the threads' sums.  Fixed
// order at every level: deterministic.
// One block (MB false): the run is all rows, and the finished sums go to out0[0] (and out1[0]).
// Many blocks (MB true; TD3 at B = 65 536: the one-block form walks 64 rows per thread, 18 - 34 us): block b takes a contiguous run of
// rows and leaves its sums in out0[b] (and out0[ERR_PARTS + b]), out0 being the partials buffer that k_finish_parts, or the FinishJob
// block of the weight-gradient summation launch (mlp_kernels.hip), adds up in block order.
template <class Row, bool MB>
__global__ void __launch_bounds__(1024) k_row_sums(int rows, const Row row, float* __restrict__ out0, float* __restrict__ out1) {
    constexpr int NS = Row::NS;
    __shared__ float red[NS][1024];
    int r0 = 0, r1 = rows;
    if constexpr (MB) {
        const int per = (rows + gridDim.x - 1) / gridDim.x;
        r0 = blockIdx.x * per;
        r1 = min(rows, r0 + per);
    }
    float s[NS] = {};
    for (int i = r0 + threadIdx.x; i < r1; i += 1024) row(i, s);
    if (Row::SUM_OPTIONAL && !out0) return;          // (uniform)
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if constexpr (MB) {
#pragma unroll
            for (int k = 0; k < NS; ++k) out0[k * ERR_PARTS + blockIdx.x] = red[k][0];
        } else {
            out0[0] = row.scale0() * red[0][0];
            if constexpr (Scale1<Row>::ANY) out1[0] = row.scale1() * red[1][0];
            else if (NS > 1) out1[0] = red[1][0];
        }
    }
}
// out0 = scale0 * sum_b part[b]; out1 (nullable) = scale1 * sum_b part[PARTS + b]
__global__ void k_finish_parts(int n_part, const float* __restrict__ part, float scale0, float scale1, float* __restrict__ out0,
                               float* __restrict__ out1) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < n_part; ++b) s += part[b];
        out0[0] = scale0 * s;
    } else if (threadIdx.x == 64 && out1) {
        float s = 0.f;
        for (int b = 0; b < n_part; ++b) s += part[ERR_PARTS + b];
        out1[0] = scale1 * s;
    }
}
// The row sums of `row` over `rows` rows into out0 (and out1): one block below ERR_MB_MIN_ROWS; from there on ERR_PARTS blocks leave
// their partials in `parts` and the finish follows - as k_finish_parts, or, where the caller has a launch_wgrad coming that can carry
// it, as the FinishJob written to *carried (left as it is otherwise: start it zeroed and pass it on if its `part` is set).
template <class Row>
int launch_row_sums(const char* name, const Row& row, int rows, float* parts, float* out0, float* out1, FinishJob* carried, hipStream_t s) {
    if (rows >= ERR_MB_MIN_ROWS) {
        const FinishJob fin{parts, ERR_PARTS, ERR_PARTS, row.scale0(), Row::NS > 1 ? Scale1<Row>::of(row) : 0.f, out0, out1};
        hipLaunchKernelGGL((k_row_sums<Row, true>), dim3(ERR_PARTS), dim3(1024), 0, s, rows, row, out0 ? parts : nullptr, (float*)nullptr);
        if (carried)
            *carried = fin;
        else if (out0)
            hipLaunchKernelGGL(k_finish_parts, dim3(1), dim3(128), 0, s, fin.n_part, fin.part, fin.scale0, fin.scale1, fin.out0, fin.out1);
    } else {
        hipLaunchKernelGGL((k_row_sums<Row, false>), dim3(1), dim3(1024), 0, s, rows, row, out0, out1);
    }
    MPG_CHECK_LAUNCH(name);
    return MPG_OK;
}

// out[i] ~ N(0, 1): Philox4x32-10(key = seed, counter = (i / 4, ctr)), Box-Muller on two of the four words per pair of outputs
// (gauss_head.h normal_pair restates one pair of it for the worker launch that draws its own)
__global__ void k_normal_fill(int n, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2, float* __restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;          // one Philox draw = four normals
    if (4 * q >= n) return;
    const Philox4 p = philox4x32_10((uint32_t)q, c1, c2, 0x6e6f726du, k0, k1);
    const float r0 = sqrtf(-2.f * logf(u01(p.v[0]))), r1 = sqrtf(-2.f * logf(u01(p.v[2])));
    float s0, c0, s1, cc1;
    sincosf(6.283185307179586f * u01(p.v[1]), &s0, &c0);
    sincosf(6.283185307179586f * u01(p.v[3]), &s1, &cc1);
    const float z[4] = {r0 * c0, r0 * s0, r1 * cc1, r1 * s1};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * q + e < n) out[4 * q + e] = z[e];
}

// the priorities' td error of TD3 (td3.py:83-92): y1 - Q1(s, a) = (y1 - y) - (Q1(s, a) - y), the last term being the `td` output of
// the critic-loss pass
__global__ void k_td3_priority(int n, const float* __restrict__ y1, const float* __restrict__ y, const float* __restrict__ td,
                               float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (y1[i] - y[i]) - td[i];
}

// ga[row][k] = dx1[row][od + k] + dx2[row][od + k]
__global__ void k_sum_action_grad(int rows, int od, int ad, const float* __restrict__ dx1, const float* __restrict__ dx2,
                                  float* __restrict__ ga) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ad) return;
    const int row = i / ad, k = i % ad;
    ga[i] = dx1[(long)row * (od + ad) + od + k] + dx2[(long)row * (od + ad) + od + k];
}

// ---- the policy head (gauss_head.h: PlainHead - the diagonal Gaussian on the logits of the policy pass - or SquashedHead, the same
// under the bijectors of an action range), one thread per row -----------------------------------------------------------------------
// logits [rows][2 ad], eps [rows][ad] -> act [rows][ad], logp [rows]; the sum of logp over the rows, where one is wanted
template <class Head>
struct HeadRow {
    int ad;
    Head head;
    const float *__restrict__ logits, *__restrict__ eps;
    float *__restrict__ act, *__restrict__ logp;
    static constexpr int NS = 1;
    static constexpr bool SUM_OPTIONAL = true;
    __host__ __device__ float scale0() const { return 1.f; }
    __device__ __forceinline__ void operator()(int i, float* s) const {
        const float lp = head.row(ad, logits + (size_t)i * 2 * ad, eps + (size_t)i * ad, act + (size_t)i * ad);
        logp[i] = lp;
        s[0] += lp;
    }
};

// HeadRow for the policy draw and, in the same pass over the same logits, the temperature's share of the batch (sac.py:138-148): the
// head's log-density under a SECOND draw eps_alpha (the reference's third compute_action: the same policy on the same observations
// through the same bijectors, only the noise differs - so no third network pass), with target_entropy added per row.  The second sum is
// finished as -inv_b * sum_rows(logp_alpha + target_entropy): this rank's share of d alpha_loss / d log_alpha.  The clipped log-std of a
// NaN logit is a bound (fmaxf / fminf return the other operand), so the plain logp_alpha is finite whatever the policy produced.
template <class Head>
struct HeadRow2 {
    int ad;
    Head head;
    const float *__restrict__ logits, *__restrict__ eps, *__restrict__ eps_alpha;
    float target_entropy, inv_b;
    float *__restrict__ act, *__restrict__ logp;
    static constexpr int NS = 2;
    static constexpr bool SUM_OPTIONAL = false;
    __host__ __device__ float scale0() const { return 1.f; }
    __host__ __device__ float scale1() const { return -inv_b; }
    __device__ __forceinline__ void operator()(int i, float* s) const {
        const float* l = logits + (size_t)i * 2 * ad;
        const float lp = head.row(ad, l, eps + (size_t)i * ad, act + (size_t)i * ad);
        logp[i] = lp;
        s[0] += lp;
        s[1] += head.logp(ad, l, eps_alpha + (size_t)i * ad) + target_entropy;
    }
};

// soft target (sac.py:78-79): y = (rew + shift) * scale + gamma * (min(q1, q2) - alpha * logp), alpha = temp() (gauss_head.h)
template <class Temp>
__global__ void k_sac_combine(int n, const float* __restrict__ rew, const float* __restrict__ q1, const float* __restrict__ q2,
                              const float* __restrict__ logp, const Temp temp, float shift, float scale, float gamma, float* __restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float alpha = temp();
    y[i] = (rew[i] + shift) * scale + gamma * (fminf(q1[i], q2[i]) - alpha * logp[i]);
}

// dL/dlogits [rows][2 ad] of loss = mean(alpha * logp - qmin) (sac.py:128) with u = mean + sigma * eps, a = u or R tanh(u):
// ga_k = dx1[row][od + k] + dx2[row][od + k] is d(-inv_b qmin)/da_k (the critics' input gradients under Td3DyRow's dy);
// mean column k: du_k = head.dsample (PlainHead: ga_k); log-std column k: du_k sigma_k eps_k - alpha inv_b, and ZERO where the clip is
// active - strictly outside [-5, 1]: clip_by_value passes the gradient at the bounds themselves (the stand-in's clamp, and TF's own
// rule).  The policy's gradient does not flow into a learned temperature (sac.py:127-128).
// The head and the temperature travel as one argument, in which an empty head takes no room (as a kernel argument of its own it would
// take a slot, and move the ones behind it).
template <class Head, class Temp>
struct HeadTemp {
    Temp temp;
    [[no_unique_address]] Head head;
};
template <class Head, class Temp>
__global__ void k_sac_dlogits(int rows, int od, int ad, const float* __restrict__ dx1, const float* __restrict__ dx2,
                              const float* __restrict__ eps, const float* __restrict__ logits, const HeadTemp<Head, Temp> ht, float inv_b,
                              float* __restrict__ dlogits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ad) return;
    const float alpha = ht.temp();
    const int row = i / ad, k = i % ad;
    const float ga = dx1[(long)row * (od + ad) + od + k] + dx2[(long)row * (od + ad) + od + k];
    const float raw = logits[(long)row * 2 * ad + ad + k];
    const bool inside = raw >= LOG_STD_MIN && raw <= LOG_STD_MAX;
    const float sigma = sigma_of(fminf(fmaxf(raw, LOG_STD_MIN), LOG_STD_MAX));
    float u = 0.f;          // (left to the optimiser, an unread u still changes the plain kernels' schedule and registers)
    if constexpr (Head::READS_U) u = mul_then_add(sigma, eps[i], logits[(long)row * 2 * ad + k]);
    const float du = ht.head.dsample(ga, u, alpha, inv_b);
    dlogits[(long)row * 2 * ad + k] = du;
    dlogits[(long)row * 2 * ad + ad + k] = inside ? du * sigma * eps[i] - alpha * inv_b : 0.f;
}

// ---- workspaces: one description each (host_glue.h Arena) ----------------------------------------------------------
struct QTargetsWs {        // mpg_q_targets, mpg_td3_targets, mpg_nstep_targets (which leaves q2 unused)
    float *a, *q1, *q2;
};
QTargetsWs q_targets_ws(Arena& ar, const mpg_cfg_t* cfg, int rows) {
    QTargetsWs w;
    w.a = ar.take((size_t)rows * cfg->act_dim);
    w.q1 = ar.take(rows);
    w.q2 = ar.take(rows);
    return w;
}

struct QLossWs {
    float *h1, *h2, *dz1, *dz2, *q, *dz3, *slabs, *parts;
};
QLossWs q_loss_ws(Arena& ar, const mpg_cfg_t* cfg, int rows) {
    QLossWs w;
    w.h1 = ar.take(stash_floats(rows)); w.h2 = ar.take(stash_floats(rows));
    w.dz1 = ar.take(stash_floats(rows)); w.dz2 = ar.take(stash_floats(rows));
    w.q = ar.take(rows); w.dz3 = ar.take(rows);
    w.slabs = ar.take(wgrad_workspace_floats(rows, cfg->obs_dim + cfg->act_dim, 1));
    w.parts = ar.take(2 * ERR_PARTS);
    return w;
}

// mpg_td3_policy_grad (two critics), mpg_dpg_policy_grad (one) and mpg_sac_policy_grad (two, with the Gaussian head): each takes only
// what it uses.  g is the policy's output gradient where a kernel forms it - the two critics' summed action gradients, or the head's
// four columns; with one critic the critic's dx serves as it is.
struct PolicyGradWs {
    float *hp1, *hp2, *h1[2], *h2[2], *dz1, *dz2, *logits, *a, *logp, *g, *dz3, *qv[2], *dy[2], *dx[2], *slabs, *parts, *lparts;
};
PolicyGradWs policy_grad_ws(Arena& ar, const mpg_cfg_t* cfg, int rows, int n_q, bool gauss) {
    const int od = cfg->obs_dim, ad = cfg->act_dim, qin = od + ad, ou = gauss ? 2 * ad : ad;
    PolicyGradWs w = {};
    w.hp1 = ar.take(stash_floats(rows)); w.hp2 = ar.take(stash_floats(rows));
    for (int k = 0; k < n_q; ++k) { w.h1[k] = ar.take(stash_floats(rows)); w.h2[k] = ar.take(stash_floats(rows)); }
    w.dz1 = ar.take(stash_floats(rows)); w.dz2 = ar.take(stash_floats(rows));
    if (gauss) { w.logits = ar.take((size_t)rows * 2 * ad); w.logp = ar.take(rows); w.lparts = ar.take(2 * ERR_PARTS); }
    w.a = ar.take((size_t)rows * ad); w.dz3 = ar.take((size_t)rows * ou);
    for (int k = 0; k < n_q; ++k) w.qv[k] = ar.take(rows);
    for (int k = 0; k < n_q; ++k) w.dy[k] = ar.take(rows);
    for (int k = 0; k < n_q; ++k) w.dx[k] = ar.take((size_t)rows * qin);
    if (n_q == 2) w.g = ar.take((size_t)rows * ou);
    w.slabs = ar.take(wgrad_workspace_floats(rows, od, 2 * ad));
    w.parts = ar.take(2 * ERR_PARTS);
    return w;
}

struct PolicySampleWs {    // mpg_policy_sample
    float* logits;
};
PolicySampleWs policy_sample_ws(Arena& ar, const mpg_cfg_t* cfg, int rows) {
    PolicySampleWs w;
    w.logits = ar.take((size_t)rows * 2 * cfg->act_dim);
    return w;
}

struct SacTargetsWs {      // mpg_sac_targets
    float *logits, *a, *logp, *q1, *q2;
};
SacTargetsWs sac_targets_ws(Arena& ar, const mpg_cfg_t* cfg, int rows) {
    SacTargetsWs w;
    w.logits = ar.take((size_t)rows * 2 * cfg->act_dim);
    w.a = ar.take((size_t)rows * cfg->act_dim);
    w.logp = ar.take(rows); w.q1 = ar.take(rows); w.q2 = ar.take(rows);
    return w;
}

// all 2 act_dim logits of the policy (MLPNet's output activation on every column; an action range never reaches them), optional stashes
OutSpec logits_out(const mpg_cfg_t* c) {
    OutSpec o = linear_out();
    o.out_tanh = c->policy_out_act == MPG_ACT_TANH;
    return o;
}
int policy_logits(const mpg_cfg_t* c, const float* params, int rows, const float* obs, float* logits, float* h1, float* h2, hipStream_t s) {
    return launch_forward(c, params, c->obs_dim, 2 * c->act_dim, 2 * c->act_dim, rows, policy_x(c, obs), logits_out(c), logits, 2 * c->act_dim,
                          h1, h2, s);
}
// The stochastic head of a call: the draws, which head, and the temperature - the caller's number, or (learned) exp(*log_alpha) read on
// the device.  The policy gradient under a learned temperature also sums the temperature's own gradient in the head's pass (AutoTemp).
struct AutoTemp {
    const float* eps_alpha;
    float target_entropy;
    float* alpha_grad;
};
struct HeadSpec {
    const float* eps;
    bool squash, learned;
    float alpha;                  // !learned (0 otherwise: the refusals' alpha test passes)
    const float* log_alpha;       // learned
    AutoTemp at;                  // learned, policy gradient only
};
HeadSpec fixed_temp(const float* eps, bool squash, float alpha) { return {eps, squash, false, alpha, nullptr, {}}; }
HeadSpec learned_temp(const float* eps, bool squash, const float* log_alpha, AutoTemp at = {}) { return {eps, squash, true, 0.f, log_alpha, at}; }

// f(the head of the call) / f(its temperature), as the types the kernels are instantiated with (gauss_head.h)
template <class F>
int with_head(const mpg_cfg_t* c, const HeadSpec& h, F f) {
    return h.squash ? f(SquashedHead{c->action_range, log_range(c->action_range)}) : f(PlainHead{});
}
template <class F>
int with_temp(const HeadSpec& h, F f) {
    return h.learned ? f(DeviceTemp{h.log_alpha}) : f(FixedTemp{h.alpha});
}
// the refusal of an entry point's family: the plain Gaussian head's, or the squashed one's
int head_refusal(bool squash, const char* entry, const mpg_cfg_t* cfg, bool pointers, int rows, float alpha) {
    return squash ? squash_refusal(entry, cfg, pointers, rows, alpha) : gauss_refusal(entry, cfg, pointers, rows, alpha);
}
template <class Describe, class... A>
size_t head_workspace_bytes(bool squash, const char* entry, const mpg_cfg_t* cfg, int rows, Describe describe, A... more) {
    return head_refusal(squash, entry, cfg, true, rows, 0.f) ? 0 : measured(describe, cfg, rows, more...);
}

// the head on `logits`: act, logp and (nullable) the sum of logp
int head_rows(const mpg_cfg_t* c, const HeadSpec& h, int rows, const float* logits, float* act, float* logp, hipStream_t s) {
    return with_head(c, h, [&](auto head) {
        return launch_row_sums("k_row_sums<HeadRow>", HeadRow<decltype(head)>{c->act_dim, head, logits, h.eps, act, logp}, rows, nullptr, nullptr,
                               nullptr, nullptr, s);
    });
}

// The policy gradient through the critic(s), td3.py:120-134 / ndpg.py:174-186 / sac.py:119-136: policy forward (a head: all 2 act_dim
// logits and the head's sample in place of the mean), the critics' forwards, dL/dq and the statistic sums, the critics' backwards down
// to dx, the policy's output gradient, the policy's backward and weight gradient.  q2 null: one critic (DPG), whose dx is dQ/da as it
// stands; Head other than NoHead (with h, temp, logp_sum): the stochastic head, two critics only (SAC).  h.at.eps_alpha non-null: the
// head's pass also sums the learned temperature's gradient into h.at.alpha_grad (HeadRow2).
struct NoHead {};          // the deterministic policy of TD3 and DPG
template <class Head, class Temp>
int policy_grad(const char* entry, const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                const HeadSpec& h, Head head, Temp temp, float inv_b, float* q_sum, float* q_sqsum, float* logp_sum, float* grad, void* ws,
                size_t ws_bytes, mpg_stream_t stream) {
    constexpr bool sampled = !std::is_same<Head, NoHead>::value;
    const int n_q = q2 ? 2 : 1;
    Arena ar(ws, ws_bytes);
    const PolicyGradWs w = policy_grad_ws(ar, cfg, rows, n_q, sampled);
    if (!ar.fits()) return workspace_too_small(entry, ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    const int od = cfg->obs_dim, ad = cfg->act_dim, qin = od + ad, ou = sampled ? 2 * ad : ad;
    // (the backward of the logits pass undoes the logits' output rule - the plain activation on every column: with an action range
    // policy_out is the DETERMINISTIC output rule, range * tanh on the mean, which the squashed head applies itself)
    const OutSpec po = std::is_same<Head, SquashedHead>::value ? logits_out(cfg) : policy_out(cfg);
    const XSpec xp = policy_x(cfg, obs);
    const float* const q[2] = {q1, q2};
    int rc;
    if constexpr (sampled) {
        rc = policy_logits(cfg, policy, rows, obs, w.logits, w.hp1, w.hp2, s);
        if (rc) return rc;
        rc = h.at.eps_alpha ? launch_row_sums("k_row_sums<HeadRow2>",
                                              HeadRow2<Head>{ad, head, w.logits, h.eps, h.at.eps_alpha, h.at.target_entropy, inv_b, w.a, w.logp},
                                              rows, w.lparts, logp_sum, h.at.alpha_grad, nullptr, s)
                            : launch_row_sums("k_row_sums<HeadRow>", HeadRow<Head>{ad, head, w.logits, h.eps, w.a, w.logp}, rows, w.lparts,
                                              logp_sum, nullptr, nullptr, s);
    } else {
        rc = policy_forward(cfg, policy, rows, xp, po, w.a, w.hp1, w.hp2, s);
    }
    if (rc) return rc;
    const XSpec xq = critic_x(cfg, obs, w.a);
    for (int k = 0; k < n_q; ++k) {
        rc = critic_forward(cfg, q[k], rows, xq, w.qv[k], w.h1[k], w.h2[k], s);
        if (rc) return rc;
    }
    // (see mpg_q_loss_grad; four used outputs have no thin form, so the head's sums are finished by k_finish_parts)
    const bool thin = backward_takes_thin(od, ou);
    FinishJob fin = {};
    rc = n_q == 2 ? launch_row_sums("k_row_sums<Td3DyRow>", Td3DyRow{w.qv[0], w.qv[1], inv_b, w.dy[0], w.dy[1]}, rows, w.parts, q_sum, q_sqsum,
                                    thin ? &fin : nullptr, s)
                  : launch_row_sums("k_row_sums<DpgDyRow>", DpgDyRow{w.qv[0], inv_b, w.dy[0]}, rows, w.parts, q_sum, q_sqsum,
                                    thin ? &fin : nullptr, s);
    if (rc) return rc;
    for (int k = 0; k < n_q; ++k) {
        rc = launch_backward(cfg, q[k], qin, 1, 1, rows, w.dy[k], 1, nullptr, 0, 0, 1.f, w.h1[k], w.h2[k], nullptr, nullptr, nullptr, w.dx[k], qin, s);
        if (rc) return rc;
    }
    // dL/d(policy output): one critic - its input gradient at the action columns (rows of qin floats, from column od on)
    const float* g = w.dx[0] + od;
    int ldg = qin;
    if (n_q == 2) {
        if constexpr (sampled)
            hipLaunchKernelGGL((k_sac_dlogits<Head, Temp>), dim3((rows * ad + 255) / 256), dim3(256), 0, s, rows, od, ad, w.dx[0], w.dx[1], h.eps,
                               w.logits, HeadTemp<Head, Temp>{temp, head}, inv_b, w.g);
        else
            hipLaunchKernelGGL(k_sum_action_grad, dim3((rows * ad + 255) / 256), dim3(256), 0, s, rows, od, ad, w.dx[0], w.dx[1], w.g);
        MPG_CHECK_LAUNCH(sampled ? "k_sac_dlogits" : "k_sum_action_grad");
        g = w.g;
        ldg = ou;
    }
    rc = launch_backward(cfg, policy, od, 2 * ad, ou, rows, g, ldg, sampled ? w.logits : w.a, ou, po.out_tanh, po.out_scale, w.hp1, w.hp2,
                         thin ? nullptr : w.dz1, w.dz2, w.dz3, nullptr, 0, s, thin ? &xp : nullptr, thin ? w.dz1 : nullptr);
    if (rc) return rc;
    return launch_wgrad(cfg, od, 2 * ad, ou, rows, xp, w.hp1, w.hp2, w.dz1, w.dz2, w.dz3, inv_b, grad, w.slabs, s, thin, thin ? w.dz1 : nullptr,
                        thin ? backward_thin_parts(rows) : 0, fin.part ? &fin : nullptr);
}

// mpg_policy_sample / mpg_policy_sample_squashed
int policy_sample(const char* entry, bool squash, const mpg_cfg_t* cfg, const float* policy, int rows, const float* obs, const float* eps,
                  float* act_out, float* logp_out, float* logits_out, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    int rc = head_refusal(squash, entry, cfg, policy && obs && eps && act_out && logp_out && ws, rows, 0.f);
    if (rc) return rc;
    Arena ar(ws, ws_bytes);
    const PolicySampleWs w = policy_sample_ws(ar, cfg, rows);
    if (!ar.fits()) return workspace_too_small(entry, ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    float* logits = logits_out ? logits_out : w.logits;
    rc = policy_logits(cfg, policy, rows, obs, logits, nullptr, nullptr, s);
    if (rc) return rc;
    return head_rows(cfg, fixed_temp(eps, squash, 0.f), rows, logits, act_out, logp_out, s);
}
// mpg_sac_targets and its _auto / _squashed forms
int sac_targets(const char* entry, const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                const float* obs_tp1, const HeadSpec& h, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    int rc = head_refusal(h.squash, entry, cfg, policy && q1t && q2t && rew && obs_tp1 && h.eps && (h.log_alpha || !h.learned) && y && ws, rows,
                          h.alpha);
    if (rc) return rc;
    Arena ar(ws, ws_bytes);
    const SacTargetsWs w = sac_targets_ws(ar, cfg, rows);
    if (!ar.fits()) return workspace_too_small(entry, ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    rc = policy_logits(cfg, policy, rows, obs_tp1, w.logits, nullptr, nullptr, s);          // sac.py:71
    if (rc) return rc;
    rc = head_rows(cfg, h, rows, w.logits, w.a, w.logp, s);
    if (rc) return rc;
    const XSpec xq = critic_x(cfg, obs_tp1, w.a);
    rc = critic_forward(cfg, q1t, rows, xq, w.q1, nullptr, nullptr, s);                     // :73
    if (rc) return rc;
    rc = critic_forward(cfg, q2t, rows, xq, w.q2, nullptr, nullptr, s);                     // :74
    if (rc) return rc;
    return with_temp(h, [&](auto temp) -> int {
        hipLaunchKernelGGL(k_sac_combine<decltype(temp)>, dim3((rows + 255) / 256), dim3(256), 0, s, rows, rew, w.q1, w.q2, w.logp, temp,
                           cfg->rew_shift, cfg->rew_scale, cfg->gamma, y);                  // :78-79
        MPG_CHECK_LAUNCH("k_sac_combine");
        return MPG_OK;
    });
}
// mpg_sac_policy_grad and its _auto / _squashed forms: mpg_td3_policy_grad with the sampled action in place of the mean - the policy
// pass keeps all its logits, the head samples, the critics' input gradients come back as in TD3 (the same dy rows: the gradient flows
// through the smaller critic), k_sac_dlogits turns them into the output gradient, and the policy's backward / weight gradient run on
// 2 act_dim outputs (the pendulum's two take the THIN backward like TD3's two actions; PathTracking's four the plain one)
int sac_policy_grad(const char* entry, const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                    const HeadSpec& h, float inv_b, float* qmin_sum, float* qmin_sqsum, float* logp_sum, float* grad, void* ws, size_t ws_bytes,
                    mpg_stream_t stream) {
    const bool temp_ok = !h.learned || (h.log_alpha && h.at.eps_alpha && h.at.alpha_grad);
    int rc = head_refusal(h.squash, entry, cfg, policy && q1 && q2 && obs && h.eps && temp_ok && qmin_sum && qmin_sqsum && logp_sum && grad && ws,
                          rows, h.alpha);
    if (rc) return rc;
    MPG_REQUIRE(!h.learned || std::isfinite(h.at.target_entropy), "%s: target_entropy must be finite (got %g)", entry,
                (double)h.at.target_entropy);
    return with_head(cfg, h, [&](auto head) {
        return with_temp(h, [&](auto temp) {
            return policy_grad(entry, cfg, policy, q1, q2, rows, obs, h, head, temp, inv_b, qmin_sum, qmin_sqsum, logp_sum, grad, ws, ws_bytes, stream);
        });
    });
}

}  // namespace

extern "C" int mpg_mlp_forward(const float* params, int in_dim, int out_dim, int out_used, int out_act, int rows,
                               const float* x, const float* in_scale, int n_scaled, float* y, const mpg_wcache_t* wcache,
                               mpg_stream_t stream) {
    MPG_REQUIRE(params && x && y && rows > 0, "mpg_mlp_forward: null pointer / rows");
    OutSpec o = linear_out();
    o.out_tanh = out_act == MPG_ACT_TANH;
    mpg_cfg_t handles = {};                    // only the handle fields are read by the launcher
    handles.wcache[0] = wcache;
    const mpg_cfg_t* cfg = &handles;
    return launch_forward(cfg, params, in_dim, out_dim, out_used, rows, xspec(x, in_dim, nullptr, 0, in_scale, n_scaled), o, y,
                          out_used, nullptr, nullptr, mpg_stream(stream));
}

extern "C" int mpg_policy_action(const mpg_cfg_t* cfg, const float* policy_params, int rows, const float* obs,
                                 float explore_sigma, uint64_t seed, uint64_t ctr, float* act, mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && policy_params && obs && act && rows > 0, "mpg_policy_action: bad argument");
    OutSpec o = policy_out(cfg);
    o.sigma = explore_sigma; o.seed = seed; o.ctr = ctr;
    return policy_forward(cfg, policy_params, rows, policy_x(cfg, obs), o, act, nullptr, nullptr, mpg_stream(stream));
}

extern "C" size_t mpg_q_targets_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    if (!net_cfg_ok(cfg) || rows <= 0) return 0;
    return measured(q_targets_ws, cfg, rows);
}

extern "C" int mpg_q_targets(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, const float* q2t, int rows,
                             const float* rew, const float* obs_tp1, const float* smooth_eps, float smooth_sigma,
                             float smooth_clip, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && policy_t && q1t && rew && obs_tp1 && y && ws && rows > 0, "mpg_q_targets: bad argument");
    Arena ar(ws, ws_bytes);
    const QTargetsWs w = q_targets_ws(ar, cfg, rows);
    if (!ar.fits()) return workspace_too_small("mpg_q_targets", ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    int rc = policy_forward(cfg, policy_t, rows, policy_x(cfg, obs_tp1), policy_out(cfg), w.a, nullptr, nullptr, s);
    if (rc) return rc;
    if (smooth_eps) {
        const int n = rows * cfg->act_dim;
        hipLaunchKernelGGL(k_smooth, dim3((n + 255) / 256), dim3(256), 0, s, n, w.a, smooth_eps, smooth_sigma, smooth_clip);
        MPG_CHECK_LAUNCH("k_smooth");
    }
    const XSpec xq = critic_x(cfg, obs_tp1, w.a);
    rc = critic_forward(cfg, q1t, rows, xq, w.q1, nullptr, nullptr, s);
    if (rc) return rc;
    if (q2t) {
        rc = critic_forward(cfg, q2t, rows, xq, w.q2, nullptr, nullptr, s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_combine_target, dim3((rows + 255) / 256), dim3(256), 0, s, rows, rew, w.q1, q2t ? w.q2 : nullptr,
                       cfg->rew_shift, cfg->rew_scale, cfg->gamma, y);
    MPG_CHECK_LAUNCH("k_combine_target");
    return MPG_OK;
}

// TD3 with prioritized replay needs TWO targets per minibatch: the clipped double-Q target with target-policy smoothing
// (td3.py:69-81) and the plain Q1 target of the priorities' td error (td3.py:83-92).  Both start from pi_t(s~'): evaluated ONCE
// here (the two mpg_q_targets calls of the method path evaluate it twice - one 65 536-row network pass, ~40 us, of every step).
extern "C" int mpg_td3_targets(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, const float* q2t, int rows,
                               const float* rew, const float* obs_tp1, const float* smooth_eps, float smooth_sigma,
                               float smooth_clip, float* y, float* y1, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && policy_t && q1t && q2t && rew && obs_tp1 && y && y1 && ws && rows > 0, "mpg_td3_targets: bad argument");
    Arena ar(ws, ws_bytes);
    const QTargetsWs w = q_targets_ws(ar, cfg, rows);
    if (!ar.fits()) return workspace_too_small("mpg_td3_targets", ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    int rc = policy_forward(cfg, policy_t, rows, policy_x(cfg, obs_tp1), policy_out(cfg), w.a, nullptr, nullptr, s);
    if (rc) return rc;
    const XSpec xq = critic_x(cfg, obs_tp1, w.a);
    rc = critic_forward(cfg, q1t, rows, xq, w.q1, nullptr, nullptr, s);      // Q1t(s~', pi_t(s~')): y1
    if (rc) return rc;
    if (smooth_eps) {
        const int n = rows * cfg->act_dim;
        hipLaunchKernelGGL(k_combine_and_smooth, dim3((n + 255) / 256), dim3(256), 0, s, rows, cfg->act_dim, rew, w.q1, cfg->rew_shift,
                           cfg->rew_scale, cfg->gamma, y1, w.a, smooth_eps, smooth_sigma, smooth_clip);
        MPG_CHECK_LAUNCH("k_combine_and_smooth");
        rc = critic_forward(cfg, q1t, rows, xq, w.q1, nullptr, nullptr, s);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_combine_target, dim3((rows + 255) / 256), dim3(256), 0, s, rows, rew, w.q1, (const float*)nullptr, cfg->rew_shift,
                           cfg->rew_scale, cfg->gamma, y1);
        MPG_CHECK_LAUNCH("k_combine_target");
    }
    rc = critic_forward(cfg, q2t, rows, xq, w.q2, nullptr, nullptr, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_combine_target, dim3((rows + 255) / 256), dim3(256), 0, s, rows, rew, w.q1, w.q2, cfg->rew_shift, cfg->rew_scale,
                       cfg->gamma, y);
    MPG_CHECK_LAUNCH("k_combine_target");
    return MPG_OK;
}

extern "C" int mpg_normal_fill(int n, uint64_t seed, uint64_t ctr, float* out, mpg_stream_t stream) {
    MPG_REQUIRE(out && n > 0, "mpg_normal_fill: bad argument");
    hipLaunchKernelGGL(k_normal_fill, dim3(((n + 3) / 4 + 255) / 256), dim3(256), 0, mpg_stream(stream), n, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32), out);
    MPG_CHECK_LAUNCH("k_normal_fill");
    return MPG_OK;
}

extern "C" int mpg_td3_priority_errors(int rows, const float* y1, const float* y, const float* td, float* out, mpg_stream_t stream) {
    MPG_REQUIRE(y1 && y && td && out && rows > 0, "mpg_td3_priority_errors: bad argument");
    hipLaunchKernelGGL(k_td3_priority, dim3((rows + 255) / 256), dim3(256), 0, mpg_stream(stream), rows, y1, y, td, out);
    MPG_CHECK_LAUNCH("k_td3_priority");
    return MPG_OK;
}

namespace {
// mpg_nstep_targets and mpg_nstep_targets_clipped: pi_t(s~_n), Q1t(s~_n, .), then the return - with `clip` the bootstrap value is
// clipped to [clip[0], clip[1]] by a kernel of its own
int nstep_targets(const char* who, const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, int rows, int n, const float* rewards,
                  const float* last_obs, const float* clip, float* y, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && policy_t && q1t && rewards && last_obs && y && ws && rows > 0 && n > 0, "%s: bad argument", who);
    Arena ar(ws, ws_bytes);
    const QTargetsWs w = q_targets_ws(ar, cfg, rows);
    if (!ar.fits()) return workspace_too_small(who, ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    int rc = policy_forward(cfg, policy_t, rows, policy_x(cfg, last_obs), policy_out(cfg), w.a, nullptr, nullptr, s);
    if (rc) return rc;
    rc = critic_forward(cfg, q1t, rows, critic_x(cfg, last_obs, w.a), w.q1, nullptr, nullptr, s);
    if (rc) return rc;
    if (clip)
        hipLaunchKernelGGL(k_nstep_clipped, dim3((rows + 255) / 256), dim3(256), 0, s, rows, n, rewards, w.q1, cfg->rew_shift,
                           cfg->rew_scale, cfg->gamma, clip[0], clip[1], y);
    else
        hipLaunchKernelGGL(k_nstep, dim3((rows + 255) / 256), dim3(256), 0, s, rows, n, rewards, w.q1, cfg->rew_shift,
                           cfg->rew_scale, cfg->gamma, y);
    MPG_CHECK_LAUNCH(clip ? "k_nstep_clipped" : "k_nstep");
    return MPG_OK;
}
}  // namespace

extern "C" int mpg_nstep_targets(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, int rows, int n,
                                 const float* rewards, const float* last_obs, float* y, void* ws, size_t ws_bytes,
                                 mpg_stream_t stream) {
    return nstep_targets("mpg_nstep_targets", cfg, policy_t, q1t, rows, n, rewards, last_obs, nullptr, y, ws, ws_bytes, stream);
}

// the pendulum's n-step target (mpg_learner.py:163-164): the bootstrap value clipped to [q_lo, q_hi] before gamma^n multiplies it
extern "C" int mpg_nstep_targets_clipped(const mpg_cfg_t* cfg, const float* policy_t, const float* q1t, int rows, int n,
                                         const float* rewards, const float* last_obs, float q_lo, float q_hi, float* y, void* ws,
                                         size_t ws_bytes, mpg_stream_t stream) {
    // (written so that a NaN bound fails it too)
    MPG_REQUIRE(q_lo >= -3.4028234664e38f && q_lo <= 3.4028234664e38f && q_hi >= -3.4028234664e38f && q_hi <= 3.4028234664e38f,
                "mpg_nstep_targets_clipped: the clip bounds must be finite (got %g, %g)", (double)q_lo, (double)q_hi);
    MPG_REQUIRE(q_lo <= q_hi, "mpg_nstep_targets_clipped: empty clip interval (q_lo %g > q_hi %g)", (double)q_lo, (double)q_hi);
    const float clip[2] = {q_lo, q_hi};
    return nstep_targets("mpg_nstep_targets_clipped", cfg, policy_t, q1t, rows, n, rewards, last_obs, clip, y, ws, ws_bytes, stream);
}

extern "C" size_t mpg_q_loss_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    if (!net_cfg_ok(cfg) || rows <= 0) return 0;
    return measured(q_loss_ws, cfg, rows);
}

extern "C" int mpg_q_loss_grad(const mpg_cfg_t* cfg, const float* q_params, int rows, const float* obs, const float* act,
                               const float* y, float inv_b_global, float* loss_sum, float* grad, float* td, void* ws,
                               size_t ws_bytes, mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && q_params && obs && act && y && loss_sum && grad && ws && rows > 0,
                "mpg_q_loss_grad: bad argument");
    Arena ar(ws, ws_bytes);
    const QLossWs w = q_loss_ws(ar, cfg, rows);
    if (!ar.fits()) return workspace_too_small("mpg_q_loss_grad", ws_bytes, ar.need);
    hipStream_t s = mpg_stream(stream);
    const int in = cfg->obs_dim + cfg->act_dim;
    const XSpec xq = critic_x(cfg, obs, act);
    int rc = critic_forward(cfg, q_params, rows, xq, w.q, w.h1, w.h2, s);
    if (rc) return rc;
    // the thin parameter gradients ride in the backward launch (mlp_launch.h): its per-workgroup partials live where the dz1 stash
    // would (never larger), the weight-gradient launch reads h1 and dz2 only
    const bool thin = backward_takes_thin(in, 1);
    // large batches: the loss partials of the many-block form are added up by one extra block of the gradient's summation launch
    // (k_finish_parts' arithmetic) when that launch exists (thin), by k_finish_parts otherwise
    FinishJob fin = {};
    rc = launch_row_sums("k_row_sums<QErrRow>", QErrRow{w.q, y, inv_b_global, w.dz3, td}, rows, w.parts, loss_sum, nullptr, thin ? &fin : nullptr, s);
    if (rc) return rc;
    rc = launch_backward(cfg, q_params, in, 1, 1, rows, w.dz3, 1, nullptr, 0, 0, 1.f, w.h1, w.h2, thin ? nullptr : w.dz1, w.dz2, nullptr, nullptr, 0, s,
                         thin ? &xq : nullptr, thin ? w.dz1 : nullptr);
    if (rc) return rc;
    return launch_wgrad(cfg, in, 1, 1, rows, xq, w.h1, w.h2, w.dz1, w.dz2, w.dz3, inv_b_global, grad, w.slabs, s, thin, thin ? w.dz1 : nullptr,
                        thin ? backward_thin_parts(rows) : 0, fin.part ? &fin : nullptr);
}

extern "C" size_t mpg_td3_policy_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    if (!net_cfg_ok(cfg) || rows <= 0) return 0;
    return measured(policy_grad_ws, cfg, rows, 2, false);
}

extern "C" int mpg_td3_policy_grad(const mpg_cfg_t* cfg, const float* policy_params, const float* q1, const float* q2,
                                   int rows, const float* obs, float inv_b_global, float* qmin_sum, float* qmin_sqsum,
                                   float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && policy_params && q1 && q2 && obs && qmin_sum && qmin_sqsum && grad && ws && rows > 0,
                "mpg_td3_policy_grad: bad argument");
    return policy_grad("mpg_td3_policy_grad", cfg, policy_params, q1, q2, rows, obs, HeadSpec{}, NoHead{}, FixedTemp{}, inv_b_global, qmin_sum,
                       qmin_sqsum, nullptr, grad, ws, ws_bytes, stream);
}

extern "C" size_t mpg_dpg_policy_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    if (!net_cfg_ok(cfg) || rows <= 0) return 0;
    return measured(policy_grad_ws, cfg, rows, 1, false);
}

// NDPGLearner.policy_forward_and_backward, ndpg.py:174-186: mpg_td3_policy_grad with ONE critic - one critic forward, one critic
// backward, and the policy's backward reads dQ/da straight out of the critic's input gradient (its last act_dim columns; there is no
// second critic to add)
extern "C" int mpg_dpg_policy_grad(const mpg_cfg_t* cfg, const float* policy_params, const float* q1, int rows, const float* obs,
                                   float inv_b_global, float* q_sum, float* q_sqsum, float* grad, void* ws, size_t ws_bytes,
                                   mpg_stream_t stream) {
    MPG_REQUIRE(net_cfg_ok(cfg) && policy_params && q1 && obs && q_sum && q_sqsum && grad && ws && rows > 0,
                "mpg_dpg_policy_grad: bad argument");
    return policy_grad("mpg_dpg_policy_grad", cfg, policy_params, q1, nullptr, rows, obs, HeadSpec{}, NoHead{}, FixedTemp{}, inv_b_global, q_sum, q_sqsum,
                       nullptr, grad, ws, ws_bytes, stream);
}

// ---- SAC: the Gaussian head (PathTracking without an action range) and, as mpg_*_squashed, the tanh-squashed one under
// cfg->action_range (PathTracking or the inverted pendulum); _auto: the learned temperature, alpha = exp(*log_alpha) read on the device.
// One body per call (policy_sample, sac_targets, sac_policy_grad above), the same launches and workspaces for every form ----
extern "C" size_t mpg_policy_sample_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    return head_workspace_bytes(false, "mpg_policy_sample_workspace_bytes", cfg, rows, policy_sample_ws);
}
extern "C" size_t mpg_policy_sample_squashed_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    return head_workspace_bytes(true, "mpg_policy_sample_squashed_workspace_bytes", cfg, rows, policy_sample_ws);
}
extern "C" size_t mpg_sac_targets_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    return head_workspace_bytes(false, "mpg_sac_targets_workspace_bytes", cfg, rows, sac_targets_ws);
}
extern "C" size_t mpg_sac_targets_squashed_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    return head_workspace_bytes(true, "mpg_sac_targets_squashed_workspace_bytes", cfg, rows, sac_targets_ws);
}
extern "C" size_t mpg_sac_policy_grad_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    return head_workspace_bytes(false, "mpg_sac_policy_grad_workspace_bytes", cfg, rows, policy_grad_ws, 2, true);
}
extern "C" size_t mpg_sac_policy_grad_squashed_workspace_bytes(const mpg_cfg_t* cfg, int rows) {
    return head_workspace_bytes(true, "mpg_sac_policy_grad_squashed_workspace_bytes", cfg, rows, policy_grad_ws, 2, true);
}

extern "C" int mpg_policy_sample(const mpg_cfg_t* cfg, const float* policy, int rows, const float* obs, const float* eps, float* act_out,
                                 float* logp_out, float* logits_out, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return policy_sample("mpg_policy_sample", false, cfg, policy, rows, obs, eps, act_out, logp_out, logits_out, ws, ws_bytes, stream);
}
extern "C" int mpg_policy_sample_squashed(const mpg_cfg_t* cfg, const float* policy, int rows, const float* obs, const float* eps,
                                          float* act_out, float* logp_out, float* logits_out, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return policy_sample("mpg_policy_sample_squashed", true, cfg, policy, rows, obs, eps, act_out, logp_out, logits_out, ws, ws_bytes, stream);
}

extern "C" int mpg_sac_targets(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                               const float* obs_tp1, const float* eps, float alpha, float* y, void* ws, size_t ws_bytes,
                               mpg_stream_t stream) {
    return sac_targets("mpg_sac_targets", cfg, policy, q1t, q2t, rows, rew, obs_tp1, fixed_temp(eps, false, alpha), y, ws, ws_bytes, stream);
}
extern "C" int mpg_sac_targets_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows, const float* rew,
                                    const float* obs_tp1, const float* eps, const float* log_alpha, float* y, void* ws, size_t ws_bytes,
                                    mpg_stream_t stream) {
    return sac_targets("mpg_sac_targets_auto", cfg, policy, q1t, q2t, rows, rew, obs_tp1, learned_temp(eps, false, log_alpha), y, ws, ws_bytes,
                       stream);
}
extern "C" int mpg_sac_targets_squashed(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows,
                                        const float* rew, const float* obs_tp1, const float* eps, float alpha, float* y, void* ws,
                                        size_t ws_bytes, mpg_stream_t stream) {
    return sac_targets("mpg_sac_targets_squashed", cfg, policy, q1t, q2t, rows, rew, obs_tp1, fixed_temp(eps, true, alpha), y, ws, ws_bytes,
                       stream);
}
extern "C" int mpg_sac_targets_squashed_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1t, const float* q2t, int rows,
                                             const float* rew, const float* obs_tp1, const float* eps, const float* log_alpha, float* y,
                                             void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return sac_targets("mpg_sac_targets_squashed_auto", cfg, policy, q1t, q2t, rows, rew, obs_tp1, learned_temp(eps, true, log_alpha), y, ws,
                       ws_bytes, stream);
}

extern "C" int mpg_sac_policy_grad(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                                   const float* eps, float alpha, float inv_b_global, float* qmin_sum, float* qmin_sqsum, float* logp_sum,
                                   float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return sac_policy_grad("mpg_sac_policy_grad", cfg, policy, q1, q2, rows, obs, fixed_temp(eps, false, alpha), inv_b_global, qmin_sum,
                           qmin_sqsum, logp_sum, grad, ws, ws_bytes, stream);
}
extern "C" int mpg_sac_policy_grad_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows, const float* obs,
                                        const float* eps, const float* log_alpha, const float* eps_alpha, float target_entropy,
                                        float inv_b_global, float* qmin_sum, float* qmin_sqsum, float* logp_sum, float* alpha_grad, float* grad,
                                        void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return sac_policy_grad("mpg_sac_policy_grad_auto", cfg, policy, q1, q2, rows, obs,
                           learned_temp(eps, false, log_alpha, {eps_alpha, target_entropy, alpha_grad}), inv_b_global, qmin_sum, qmin_sqsum,
                           logp_sum, grad, ws, ws_bytes, stream);
}
extern "C" int mpg_sac_policy_grad_squashed(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows,
                                            const float* obs, const float* eps, float alpha, float inv_b_global, float* qmin_sum,
                                            float* qmin_sqsum, float* logp_sum, float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return sac_policy_grad("mpg_sac_policy_grad_squashed", cfg, policy, q1, q2, rows, obs, fixed_temp(eps, true, alpha), inv_b_global, qmin_sum,
                           qmin_sqsum, logp_sum, grad, ws, ws_bytes, stream);
}
extern "C" int mpg_sac_policy_grad_squashed_auto(const mpg_cfg_t* cfg, const float* policy, const float* q1, const float* q2, int rows,
                                                 const float* obs, const float* eps, const float* log_alpha, const float* eps_alpha,
                                                 float target_entropy, float inv_b_global, float* qmin_sum, float* qmin_sqsum, float* logp_sum,
                                                 float* alpha_grad, float* grad, void* ws, size_t ws_bytes, mpg_stream_t stream) {
    return sac_policy_grad("mpg_sac_policy_grad_squashed_auto", cfg, policy, q1, q2, rows, obs,
                           learned_temp(eps, true, log_alpha, {eps_alpha, target_entropy, alpha_grad}), inv_b_global, qmin_sum, qmin_sqsum,
                           logp_sum, grad, ws, ws_bytes, stream);
}
