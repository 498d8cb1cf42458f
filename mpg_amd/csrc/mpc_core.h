// The MPC baseline's device code, shared by mpc_kernels.hip (mpg_mpc_cost_grad, mpg_mpc_solve) and env_path_tracking.hip
// (mpg_mpc_rollout): the horizon cost ModelPredictiveControl.cost_function (mpc/main.py:156-165), its gradient by a hand adjoint, and a
// whole spectral projected gradient solve (Birgin, Martinez, Raydan 2000) per lane.  include/mpg_hip.h states the problem, the method
// and its constants.  A namespace of its own: the vehicle constants below are the model's at tau = 0.1, the env's (tau = 0.005) carry
// the same names.
//
// One lane = one row, workgroups of one wave.  A lane's arrays - controls, gradient, trial point, the stored states of the last forward
// pass - are indexed by the running step, so they live in LDS as [index][lane]: a wave's 64 lanes read 64 consecutive dwords, one per
// bank, and nothing is addressed through a private array (which would be scratch: build.py keeps allocas out of LDS).  11 * horizon
// floats per lane for the solver (22 KiB .. 85 KiB per workgroup), 9 * horizon for the cost.  Entry 5 of the state, x, never reaches the
// cost: it is carried for `traj` only and has no adjoint.
//
// This is NOT rollout::PathTracking::step (rollout_common.h): the steer scale is 0.4, not 1.2 pi / 9; delta_y has no 0.5 + 0.01 eps term;
// entry 0 is the speed itself, not speed - 20.  The adjoint has that one's structure, the gate on the v_x clamp included.  As there the
// reciprocal, sine and cosine are the hardware's (<= 1-2 ulp).  No contraction: the forward pass is one inlined function, and the bits
// of a cost must not depend on which kernel it was inlined into (mpg_mpc_solve's cost_out is mpg_mpc_cost_grad's at the returned u, and
// mpg_mpc_rollout's solves are mpg_mpc_solve's).
#pragma once
#include <math.h>

#include "mpg_common.h"

#pragma clang fp contract(off)

namespace mpc {

constexpr int WAVE = 64;
constexpr int NX = 5;                    // stored state entries per step: v_x, v_y, r, delta_y, delta_phi
// vehicle parameters, mpc/main.py:60-67; tau = 1 / base_frequency = 0.1 (:116)
constexpr float C_f = -128915.5f, C_r = -85943.6f, A = 1.06f, B = 1.85f, MASS = 1412.f, I_z = 1536.7f, TAU = 0.1f;
constexpr float K1 = TAU * (A * C_f - B * C_r), K2 = TAU * C_f, K3 = TAU * MASS, K4 = TAU * (C_f + C_r);
constexpr float K5 = TAU * A * C_f, K6 = TAU * (A * A * C_f + B * B * C_r);
constexpr float PI_F = 3.14159265358979323846f;
constexpr float EXPECTED_VS = 20.f;      // :118

struct State {
    float vx, vy, r, dy, dphi, x;
};

// np.clip forms: a NaN passes through (fminf / fmaxf would turn it into a bound)
__device__ __forceinline__ float box(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ float clip_vx(float v) { return v < 1.f ? 1.f : (v > 35.f ? 35.f : v); }
__device__ __forceinline__ float raw_next_vx(float vx, float vy, float r, float ax) { return vx + TAU * (ax + vy * r); }

// cost_function :156-165 from x0 with the controls P[j * WAVE], j < 2 * H.  Stores the state BEFORE step i at X[(NX * i + e) * WAVE] and,
// for a non-null traj, x_0 .. x_H at traj[6 * i + e].
__device__ __forceinline__ float forward(int H, const State& x0, const float* P, float* X, float* traj) {
    State s = x0;
    float cost = 0.f;
    for (int i = 0; i < H; ++i) {
        const float de = P[(2 * i) * WAVE] * MPG_MPC_STEER_SCALE, ax = P[(2 * i + 1) * WAVE] * MPG_MPC_ACC_SCALE;
        float* xs = X + NX * i * WAVE;
        xs[0 * WAVE] = s.vx; xs[1 * WAVE] = s.vy; xs[2 * WAVE] = s.r; xs[3 * WAVE] = s.dy; xs[4 * WAVE] = s.dphi;
        if (traj) {
            float* t = traj + 6 * i;
            t[0] = s.vx; t[1] = s.vy; t[2] = s.r; t[3] = s.dy; t[4] = s.dphi; t[5] = s.x;
        }
        // compute_rew :128-143, negated
        const float dv = s.vx - EXPECTED_VS;
        cost += 0.01f * (dv * dv) + 0.04f * (s.dy * s.dy) + 0.1f * (s.dphi * s.dphi) + 0.02f * (s.r * s.r) + 5.f * (de * de) +
                0.05f * (ax * ax);
        // f_xu :75-104 at tau = 0.1
        const float iD1 = __builtin_amdgcn_rcpf(MASS * s.vx - K4), iD2 = __builtin_amdgcn_rcpf(K6 - I_z * s.vx);
        const float sp = __sinf(s.dphi), cp = __cosf(s.dphi);
        State n;
        n.vx = clip_vx(raw_next_vx(s.vx, s.vy, s.r, ax));                                              // :149
        n.vy = (MASS * s.vy * s.vx + K1 * s.r - K2 * de * s.vx - K3 * s.vx * s.vx * s.r) * iD1;
        n.r = (-I_z * s.r * s.vx - K1 * s.vy + K5 * de * s.vx) * iD2;
        n.dy = s.dy + TAU * (s.vx * sp + s.vy * cp);
        n.dphi = s.dphi + TAU * s.r;
        if (n.dphi > PI_F) n.dphi -= 2.f * PI_F;                                                       // :150
        if (n.dphi <= -PI_F) n.dphi += 2.f * PI_F;                                                     // :151
        n.x = s.x + TAU * (s.vx * cp - s.vy * sp);
        s = n;
    }
    if (traj) {
        float* t = traj + 6 * H;
        t[0] = s.vx; t[1] = s.vy; t[2] = s.r; t[3] = s.dy; t[4] = s.dphi; t[5] = s.x;
    }
    return cost;
}

// The reverse pass over the states X of the last forward pass, which was taken at the point P.  d cost / d (normalised control j) goes to
// G[j * WAVE]; pg = max_j |box(P_j - g_j) - P_j|, a NaN kept.  UPDATE (the solver's accepted step, P = the trial point T): before G[j] is
// overwritten s_j = P_j - U_j and y_j = g_j - G[j] enter ss = <s, s> and sy = <s, y>, and U_j becomes P_j.
template <bool UPDATE>
__device__ __forceinline__ void reverse(int H, const float* P, const float* X, float* U, float* G, float& pg, float& ss, float& sy) {
    float l_vx_in = 0.f, l_vy = 0.f, l_r = 0.f, l_dy = 0.f, l_dphi = 0.f;      // adjoint of the state behind step i
    pg = 0.f; ss = 0.f; sy = 0.f;
    auto commit = [&](int j, float gnew) {
        const float p = P[j * WAVE];
        if (UPDATE) {
            const float s = p - U[j * WAVE], y = gnew - G[j * WAVE];
            ss += s * s;
            sy += s * y;
            U[j * WAVE] = p;
        }
        G[j * WAVE] = gnew;
        const float v = fabsf(box(p - gnew) - p);
        pg = (pg != pg) ? pg : (!(v <= pg) ? v : pg);
    };
    for (int i = H - 1; i >= 0; --i) {
        const float* xs = X + NX * i * WAVE;
        const float vx = xs[0 * WAVE], vy = xs[1 * WAVE], r = xs[2 * WAVE], dy = xs[3 * WAVE], dphi = xs[4 * WAVE];
        const float de = P[(2 * i) * WAVE] * MPG_MPC_STEER_SCALE, ax = P[(2 * i + 1) * WAVE] * MPG_MPC_ACC_SCALE;
        const float nvx_raw = raw_next_vx(vx, vy, r, ax);
        const float l_vx = (nvx_raw >= 1.f && nvx_raw <= 35.f) ? l_vx_in : 0.f;      // np.clip passes no gradient outside its bounds
        const float iD1 = __builtin_amdgcn_rcpf(MASS * vx - K4), iD2 = __builtin_amdgcn_rcpf(K6 - I_z * vx);
        const float nvy = (MASS * vy * vx + K1 * r - K2 * de * vx - K3 * vx * vx * r) * iD1;
        const float nr = (-I_z * r * vx - K1 * vy + K5 * de * vx) * iD2;
        const float sp = __sinf(dphi), cp = __cosf(dphi);
        const float dvy_vx = (MASS * vy - K2 * de - 2.f * K3 * vx * r - nvy * MASS) * iD1;
        const float dvy_vy = MASS * vx * iD1;
        const float dvy_r = (K1 - K3 * vx * vx) * iD1;
        const float dvy_de = -K2 * vx * iD1;
        const float dr_vx = (-I_z * r + K5 * de + nr * I_z) * iD2;
        const float dr_vy = -K1 * iD2;
        const float dr_r = -I_z * vx * iD2;
        const float dr_de = K5 * vx * iD2;
        // (the wrap of delta_phi is a shift: derivative 1; x has no adjoint)
        const float g_vx = l_vx + l_vy * dvy_vx + l_r * dr_vx + l_dy * TAU * sp + 0.02f * (vx - EXPECTED_VS);
        const float g_vy = l_vx * TAU * r + l_vy * dvy_vy + l_r * dr_vy + l_dy * TAU * cp;
        const float g_r = l_vx * TAU * vy + l_vy * dvy_r + l_r * dr_r + l_dphi * TAU + 0.04f * r;
        const float g_dy = l_dy + 0.08f * dy;
        const float g_dphi = l_dphi + l_dy * TAU * (vx * cp - vy * sp) + 0.2f * dphi;
        commit(2 * i + 1, (l_vx * TAU + 0.1f * ax) * MPG_MPC_ACC_SCALE);
        commit(2 * i, (l_vy * dvy_de + l_r * dr_de + 10.f * de) * MPG_MPC_STEER_SCALE);
        l_vx_in = g_vx; l_vy = g_vy; l_r = g_r; l_dy = g_dy; l_dphi = g_dphi;
    }
}

// lanes behind the last row work on a harmless state and store nothing
__device__ __forceinline__ State idle_state() { return State{EXPECTED_VS, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// what a solve leaves beside the point itself (in U)
struct Solved {
    float cost, pgnorm;
    int info;                                   // accepted iterations k, or -(k + 1) behind a failed line search
};

// mpg_mpc_solve's problem for one lane, as solve() below takes a problem: the number of controls, forward(P) = the cost at the point P
// (which leaves what the reverse pass needs), and reverse<UPDATE>(P, U, G, pg, ss, sy) with the contract of the function above.
struct PathProblem {
    int H;
    const State& s0;
    float* X;                                   // the states of the last forward pass [NX H][WAVE]
    __device__ __forceinline__ int controls() const { return 2 * H; }
    __device__ __forceinline__ float forward(const float* P) const { return mpc::forward(H, s0, P, X, nullptr); }
    template <bool UPDATE>
    __device__ __forceinline__ void reverse(const float* P, float* U, float* G, float& pg, float& ss, float& sy) const {
        mpc::reverse<UPDATE>(H, P, X, U, G, pg, ss, sy);
    }
};

// One whole solve of the method of mpg_mpc_solve for this lane's row of the problem `prob` (PathProblem above; model_mpc.h has the
// learners' models) from the start point the caller left in U, ALREADY inside the box.  The lane's arrays of prob.controls() floats
// each, [index][WAVE]: U the last accepted point (the solution on return), G its gradient, T the trial point.  A lane with `valid`
// false (behind the last row) takes part in the wave's control flow only.
template <class PROB>
__device__ __forceinline__ Solved solve(const PROB& prob, int iters, float tol, bool valid, float* U, float* G, float* T) {
    const int n = prob.controls();
    float f = prob.forward(U);
    float pg, ss, sy;
    prob.template reverse<false>(U, U, G, pg, ss, sy);

    // the last MPG_MPC_SPG_M accepted costs, newest first, as named registers (an array indexed by k % M would be scratch)
    static_assert(MPG_MPC_SPG_M == 5, "the cost history below is written out for M = 5");
    float h0 = f, h1 = -INFINITY, h2 = -INFINITY, h3 = -INFINITY, h4 = -INFINITY;
    float alpha = MPG_MPC_SPG_ALPHA0;
    int accepted = 0, failed = 0;
    bool live = valid && !(tol > 0.f && pg <= tol);
    // Every loop below has a fixed trip bound and leaves early only on a condition the whole wave shares; a lane that is done is
    // masked out of the work, it takes no exit of its own.
    for (int k = 0; k < iters; ++k) {
        if (!__any(live)) break;
        float gd = 0.f;
        if (live)
            // (by four in every kernel this is inlined into: left to itself the compiler unrolled it in k_mpc_solve and not in
            // k_mpc_rollout, where every element then waited out its own LDS round trip)
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const float uj = U[j * WAVE], gj = G[j * WAVE];
                gd += gj * (box(uj - alpha * gj) - uj);
            }
        const float fmax = fmaxf(fmaxf(fmaxf(h0, h1), fmaxf(h2, h3)), h4);      // h0 is never NaN behind an accepted step
        float lambda = 1.f, fnew = f;
        bool searching = live;
        for (int h = 0; h <= MPG_MPC_SPG_HALVINGS; ++h) {
            if (!__any(searching)) break;
            if (searching) {
                for (int j = 0; j < n; ++j) {
                    const float uj = U[j * WAVE], gj = G[j * WAVE];
                    T[j * WAVE] = box(uj + lambda * (box(uj - alpha * gj) - uj));
                }
                const float ft = prob.forward(T);
                if (ft <= fmax + MPG_MPC_SPG_GAMMA * lambda * gd) {
                    searching = false;
                    fnew = ft;
                } else {
                    lambda *= 0.5f;
                }
            }
        }
        if (live && searching) {                // nothing accepted: the row keeps U, f and pg
            live = false;
            failed = 1;
        }
        if (live) {
            prob.template reverse<true>(T, U, G, pg, ss, sy);
            alpha = sy > 0.f ? ss / sy : MPG_MPC_SPG_ALPHA_MAX_STEP;
            alpha = fminf(fmaxf(alpha, MPG_MPC_SPG_ALPHA_LO), MPG_MPC_SPG_ALPHA_HI);
            f = fnew;
            h4 = h3; h3 = h2; h2 = h1; h1 = h0; h0 = f;
            ++accepted;
            if (tol > 0.f && pg <= tol) live = false;
        }
    }
    return Solved{f, pg, failed ? -(accepted + 1) : accepted};
}

// mpg_mpc_solve's own problem; X: the states of the last forward pass [NX H][WAVE]
__device__ __forceinline__ Solved solve(int H, int iters, float tol, bool valid, const State& s0, float* U, float* G, float* T, float* X) {
    return solve(PathProblem{H, s0, X}, iters, tol, valid, U, G, T);
}

// LDS of one workgroup: n_arrays_of_2H lane arrays of 2 H floats and the stored states
inline size_t lds_bytes(int H, int n_arrays_of_2H) { return (size_t)(2 * n_arrays_of_2H + NX) * H * WAVE * sizeof(float); }

// more than 64 KiB of dynamic LDS is asked for by name, kernel by kernel (the device has 160 KiB per CU)
template <class K>
int allow_lds(const char* entry, K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return MPG_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        mpg_set_error("%s: %zu bytes of LDS: %s", entry, bytes, hipGetErrorString(e));
        return -(int)e;
    }
    return MPG_OK;
}

}  // namespace mpc
