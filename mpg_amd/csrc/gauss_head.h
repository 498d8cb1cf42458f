// Gaussian policy head (policy.py:179-204: MultivariateNormalDiag(mean, exp(clip(log_std, -5, 1))); with action_range None no bijector,
// with one the tanh-squashed sibling further down) on the 2 act_dim logits of the policy pass, and the element function of the library's standard-normal stream.  Shared by the two
// translation units that evaluate the head - learner_api.hip (k_row_sums<HeadRow<Head>>, k_sac_dlogits<Head, Temp>) and env_path_tracking.hip (the
// stochastic worker launch) - which must agree bit for bit: include it where contraction is allowed (env_path_tracking.hip: inside
// its `#pragma clang fp contract(fast)` block), so that both compile these expressions under the same rule.
#pragma once
#include <math.h>

#include "mpg_common.h"

namespace gauss {

constexpr float LOG_STD_MIN = -5.f, LOG_STD_MAX = 1.f, HALF_LOG_2PI = 0.91893853320467274f;
// sigma = exp(log_std) as the CORRECTLY ROUNDED float32 exponential (the double-precision exp, rounded once): the float32 library exp is
// within an ulp of it and its last bit differs between compiler versions, while a sample must be reproducible from logits_out by anyone
// (two values per row: the double-precision pipe is not on any hot path here)
__device__ __forceinline__ float sigma_of(float clipped_log_std) { return (float)exp((double)clipped_log_std); }
// a * b + c with the product and the sum rounded separately, whatever the translation unit's contraction mode (the __fmul_rn / __fadd_rn
// intrinsics are plain operators here and fuse)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return p + c;
}
// act = mean + sigma * eps with the product and the sum rounded separately (the same bits as the two-op expression a caller forms
// from logits_out); returns the row's log-density.  z, the standardised sample of the density, is eps ITSELF: TFP forms
// (a - mean) / sigma, which in exact arithmetic is eps and in float32 is eps with two more roundings - against the float64 run of the
// reference, where that expression returns eps to 1e-16, eps is the nearer of the two.
__device__ __forceinline__ float gauss_row(int ad, const float* __restrict__ l, const float* __restrict__ e, float* __restrict__ a) {
    float lp = 0.f;
    for (int k = 0; k < ad; ++k) {
        const float ls = fminf(fmaxf(l[ad + k], LOG_STD_MIN), LOG_STD_MAX), sigma = sigma_of(ls), z = e[k];
        a[k] = mul_then_add(sigma, z, l[k]);
        lp += (-0.5f * z * z - ls) - HALF_LOG_2PI;
    }
    return lp;
}
// the log-density alone of the same head under another draw `e` (no action written): gauss_row's terms in gauss_row's order, so that
// on the same draw it returns gauss_row's bits (the temperature's gradient, sac.py:138-148, needs logp of a draw nobody acts with)
__device__ __forceinline__ float gauss_logp(int ad, const float* __restrict__ l, const float* __restrict__ e) {
    float lp = 0.f;
    for (int k = 0; k < ad; ++k) {
        const float ls = fminf(fmaxf(l[ad + k], LOG_STD_MIN), LOG_STD_MAX), z = e[k];
        lp += (-0.5f * z * z - ls) - HALF_LOG_2PI;
    }
    return lp;
}
// ---- the tanh-squashed head (policy.py:183-190 with an action_range R: the same diagonal Gaussian under Chain([Affine(R), Tanh()])) ----
// act = R tanh(u), u = mean + sigma * eps formed as gauss_row forms it;
// logp = [gauss_row's sum] - sum_k 2 (log 2 - u_k - softplus(-2 u_k)) - ad log R: the Tanh bijector's published
// forward_log_det_jacobian and Affine's.  The density is evaluated at u ITSELF, not at atanh(act / R): TFP's bijector cache returns the
// x that produced y when log_prob is called on the tensor sample() returned - the decision of z = eps in gauss_row, for its reason
// (and atanh of a saturated act is infinite where u is merely large).
// tanh_ldj(u) = 2 (log 2 - u - softplus(-2 u)) = log(1 - tanh(u)^2), an even function: evaluated at |u|, where softplus(-2 |u|) =
// log1p(exp(-2 |u|)) has an argument in (0, 1] - no overflow at any u, and no difference of two large terms on the negative side
constexpr float LOG_2 = 0.69314718055994531f;
__device__ __forceinline__ float tanh_ldj(float u) {
    const float au = fabsf(u);
    return 2.f * ((LOG_2 - au) - log1pf(expf(-2.f * au)));
}
// 1 - tanh(u)^2 = 4 e / (1 + e)^2 with e = exp(-2 |u|): no cancellation where tanh saturates
__device__ __forceinline__ float sech2(float u) {
    const float e = expf(-2.f * fabsf(u)), d = 1.f + e;
    return 4.f * e / (d * d);
}
// log R of the Affine bijector as the correctly rounded float32 logarithm (sigma_of's rule), formed on the host
inline float log_range(float range) { return (float)log((double)range); }
// gauss_row under the bijectors: a[k] = range * tanh(u_k); returns the squashed log-density
__device__ __forceinline__ float squash_row(int ad, float range, float log_r, const float* __restrict__ l, const float* __restrict__ e,
                                            float* __restrict__ a) {
    float lp = 0.f, ldj = 0.f;
    for (int k = 0; k < ad; ++k) {
        const float ls = fminf(fmaxf(l[ad + k], LOG_STD_MIN), LOG_STD_MAX), sigma = sigma_of(ls), z = e[k];
        const float u = mul_then_add(sigma, z, l[k]);
        a[k] = range * tanhf(u);
        lp += (-0.5f * z * z - ls) - HALF_LOG_2PI;
        ldj += tanh_ldj(u);
    }
    return (lp - ldj) - (float)ad * log_r;
}
// the squashed log-density alone under another draw (gauss_logp's role): squash_row's terms in squash_row's order
__device__ __forceinline__ float squash_logp(int ad, float log_r, const float* __restrict__ l, const float* __restrict__ e) {
    float lp = 0.f, ldj = 0.f;
    for (int k = 0; k < ad; ++k) {
        const float ls = fminf(fmaxf(l[ad + k], LOG_STD_MIN), LOG_STD_MAX), sigma = sigma_of(ls), z = e[k];
        lp += (-0.5f * z * z - ls) - HALF_LOG_2PI;
        ldj += tanh_ldj(mul_then_add(sigma, z, l[k]));
    }
    return (lp - ldj) - (float)ad * log_r;
}

// ---- the head as a type: what a kernel that serves both heads is instantiated with.  row / logp are the functions above; dsample is
// dL/du of loss = mean(alpha * logp - qmin) at the pre-bijector sample u = mean + sigma * eps of one column, given
// ga = d(-inv_b qmin)/da.  Plain: a = u, so ga, and u is not looked at (READS_U: the caller need not form it).  Squashed: a = R tanh(u)
// and logp = ... - log(1 - tanh(u)^2) - log R, so ga R (1 - t^2) + 2 alpha inv_b t (t = tanh u).
struct PlainHead {
    static constexpr bool READS_U = false;
    __device__ __forceinline__ float row(int ad, const float* __restrict__ l, const float* __restrict__ e, float* __restrict__ a) const {
        return gauss_row(ad, l, e, a);
    }
    __device__ __forceinline__ float logp(int ad, const float* __restrict__ l, const float* __restrict__ e) const { return gauss_logp(ad, l, e); }
    __device__ __forceinline__ float dsample(float ga, float, float, float) const { return ga; }
};
struct SquashedHead {
    static constexpr bool READS_U = true;
    float range, log_r;
    __device__ __forceinline__ float row(int ad, const float* __restrict__ l, const float* __restrict__ e, float* __restrict__ a) const {
        return squash_row(ad, range, log_r, l, e, a);
    }
    __device__ __forceinline__ float logp(int ad, const float* __restrict__ l, const float* __restrict__ e) const {
        return squash_logp(ad, log_r, l, e);
    }
    __device__ __forceinline__ float dsample(float ga, float u, float alpha, float inv_b) const {
        return ga * range * sech2(u) + 2.f * alpha * inv_b * tanhf(u);
    }
};

// alpha = exp(log_alpha) of the learned temperature, under sigma_of's rule and for its reason: the correctly rounded float32
// exponential, which anyone can re-form on the host bit for bit
__device__ __forceinline__ float alpha_of(const float* __restrict__ log_alpha) { return (float)exp((double)*log_alpha); }
// ---- the temperature as a type: the caller's number, or the learned one read on the device
struct FixedTemp {
    float alpha;
    __device__ __forceinline__ float operator()() const { return alpha; }
};
struct DeviceTemp {
    const float* __restrict__ log_alpha;
    __device__ __forceinline__ float operator()() const { return alpha_of(log_alpha); }
};

// Elements 4 q + 2 pair and 4 q + 2 pair + 1 of the stream mpg_normal_fill writes for (key, counter): Philox block q, Box-Muller on
// the words (v[0], v[1]) (pair 0) or (v[2], v[3]) (pair 1) - the cosine for the even element, the sine for the odd one.  k_normal_fill
// (learner_api.hip) states the same operations for a whole block; tests/test_sac_native_gpu.py compares the two bit for bit.
// The logarithm and the root are the builtins themselves, not the library's logf / sqrtf: those are wrappers that the HIP headers
// define ahead of any pragma, so the backend would expand them under the translation unit's own contraction mode (the last step of
// the logarithm's expansion is a product and a sum that fuse under one mode and not under the other), while a builtin called HERE is
// expanded under the mode in force here - which is k_normal_fill's.
constexpr uint32_t NORMAL_STREAM_TAG = 0x6e6f726du;
__device__ __forceinline__ void normal_pair(uint32_t q, int pair, uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2, float& z_even,
                                            float& z_odd) {
    const Philox4 p = philox4x32_10(q, c1, c2, NORMAL_STREAM_TAG, k0, k1);
    const uint32_t a = pair ? p.v[2] : p.v[0], b = pair ? p.v[3] : p.v[1];     // selects: never a run-time index (mpg_common.h)
    const float r = __builtin_sqrtf(-2.f * __builtin_logf(u01(a)));
    float s, c;
    sincosf(6.283185307179586f * u01(b), &s, &c);
    z_even = r * c;
    z_odd = r * s;
}

// The refusals the Gaussian-head entry points (and their workspace queries) share, in the order include/mpg_hip.h lists them.
// `entry` names the caller in every message; MPG_OK when the call may proceed.  (The width test is what net_cfg_ok, host_glue.h,
// leaves once act_dim is 2 and there is no action range.)
inline int gauss_refusal(const char* entry, const mpg_cfg_t* cfg, bool pointers, int rows, float alpha) {
    MPG_REQUIRE(cfg && pointers, "%s: null pointer", entry);
    MPG_REQUIRE(rows > 0, "%s: rows must be positive (got %d)", entry, rows);
    MPG_REQUIRE(cfg->act_dim == 2 && cfg->env_kind == MPG_ENV_PATH_TRACKING,
                "%s: Gaussian head without an action range only (act_dim 2 on PathTracking; got act_dim %d, env_kind %d)", entry,
                cfg->act_dim, cfg->env_kind);
    MPG_REQUIRE(!(cfg->action_range > 0.f), "%s: Gaussian head without an action range only (got action_range %g)", entry,
                (double)cfg->action_range);
    MPG_REQUIRE(cfg->obs_dim >= 6 && cfg->obs_dim <= 16, "%s: unsupported observation width %d", entry, cfg->obs_dim);
    MPG_REQUIRE(alpha >= 0.f && alpha <= 3.4028234664e38f, "%s: alpha must be finite and not negative (got %g)", entry, (double)alpha);
    return MPG_OK;
}

// The refusals of the squashed entry points (mpg_*_squashed and their queries), each with a text of its own: PathTracking (act_dim 2,
// obs_dim 6 .. 16) or the inverted pendulum (act_dim 1, obs_dim 4), a positive action range over a linear output.
inline int squash_refusal(const char* entry, const mpg_cfg_t* cfg, bool pointers, int rows, float alpha) {
    MPG_REQUIRE(cfg && pointers, "%s: null pointer", entry);
    MPG_REQUIRE(rows > 0, "%s: rows must be positive (got %d)", entry, rows);
    MPG_REQUIRE(cfg->env_kind != MPG_ENV_INVERTED_DOUBLE_PENDULUM, "%s: the squashed head is not built for the double pendulum (env_kind %d)",
                entry, cfg->env_kind);
    MPG_REQUIRE((cfg->act_dim == 2 && cfg->env_kind == MPG_ENV_PATH_TRACKING) || (cfg->act_dim == 1 && cfg->env_kind == MPG_ENV_INVERTED_PENDULUM),
                "%s: squashed head on PathTracking (act_dim 2) or the inverted pendulum (act_dim 1) only (got act_dim %d, env_kind %d)", entry,
                cfg->act_dim, cfg->env_kind);
    MPG_REQUIRE(cfg->action_range > 0.f && cfg->action_range <= 3.4028234664e38f,
                "%s: the squashed head needs a positive, finite action range (got action_range %g)", entry, (double)cfg->action_range);
    MPG_REQUIRE(cfg->policy_out_act != MPG_ACT_TANH, "%s: a tanh output activation under an action range is not built (range * tanh(tanh(z)))",
                entry);
    MPG_REQUIRE(cfg->act_dim == 2 ? (cfg->obs_dim >= 6 && cfg->obs_dim <= 16) : cfg->obs_dim == 4, "%s: unsupported observation width %d", entry,
                cfg->obs_dim);
    MPG_REQUIRE(alpha >= 0.f && alpha <= 3.4028234664e38f, "%s: alpha must be finite and not negative (got %g)", entry, (double)alpha);
    return MPG_OK;
}

}  // namespace gauss
