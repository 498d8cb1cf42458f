// The policy pass as the env translation units run it inside their own launches (env_path_tracking.hip, env_cart_pole.hip): what a
// 512-thread workgroup does for ONE 16-row group of mpg_policy_action / policy_logits - k_forward<IN, OU, PK, 1> (mlp_kernels.hip) for
// that unit: the same device functions on the same operands in the same order, so the values are bit-identical to the stand-alone
// launch's - cut into the pieces those kernels compose.  Include inside a `#pragma clang fp contract(fast)` block, as mlp_core.h.
//
// THE RESIDENT PLAN (the one-launch rollouts of both files): one 512-thread workgroup owns a 16-agent group for all iterations.  The
// policy's registers are loaded once (load), wave 0 holds the agents in registers, and per iteration the observations go from wave 0
// to the pass (stage) and the actions back through LDS between workgroup barriers.  Global memory is read in the prologue only and
// written, never read back; zmax / saw_nan accumulate over the passes and report() ORs them into the status word once.
//
// These kernels have NO REGISTER HEADROOM (k_eval_rollout, k_worker_sample_rollout: 254 - 256 VGPRs), and their instructions follow the
// ORDER of the statements here and how deep a piece is nested: the pieces are forced inline and called from the kernels directly.  After
// an edit compare tools/asm.py's output and run tools/kernel_resources.py on both files.
#pragma once
#include "mlp_core.h"

namespace policy_pass {
using namespace mlp;

// (OU: the used outputs the pass is built for)
template <int IN, int OU>
__host__ __device__ constexpr int smem_floats() { return A_IMG + GROUP * xs_of<IN>() + NWAVE * GROUP * out_stride<OU>(); }

// (A: a kernel's policy arguments - params, pack (nullable: the packed forward image of W2), scale: obs_scale, status - with
// obs_dim_of(a), the network's input width, in A's own namespace: it is read here, where the kernels read it.)
// The policy's registers: the lane's bias b3v (lane tid < 16 OU forms output tid % OU of row tid / OU), the small operands, W2.
template <bool PK, int IN, int OU, class A>
__device__ __forceinline__ void load(const A& a, int out_dim, const Lane& L, float (&w2)[128], SmallRegs<IN, OU>& r, float& b3v) {
    const Net net = make_net(a.params, obs_dim_of(a), out_dim);
    b3v = 0.f;
    if (threadIdx.x < GROUP * OU) b3v = net.b3[threadIdx.x % OU];
    load_small<IN, OU>(net, L, r);
    if constexpr (PK) load_w2_packed(a.pack, L, w2); else load_w2_fwd(net.W2, L, w2);
}

// From the scaled inputs sX [16][XS] the lanes have just written (smem + A_IMG) to the output partials (smem + A_IMG + 16 XS):
// returns the lane's row_poison term.
template <int IN, int OU>
__device__ __forceinline__ float forward(float* smem, const Lane& L, const float (&w2)[128], const SmallRegs<IN, OU>& r, float& zmax) {
    constexpr int XSW = xs_of<IN>();
    float* sA = smem;
    float* sX = sA + A_IMG;
    float* sPart = sX + GROUP * XSW;
    lds_barrier();
    float pz = 0.f;
    if (threadIdx.x < GROUP * OU) pz = row_poison(sX + (threadIdx.x / OU) * XSW, XSW);
    float h1[2][4], h2[2][4];
    forward_group<IN, OU>(sX, sA, sPart, L, w2, r, h1, h2, nullptr, 0, nullptr, &zmax);
    return pz;
}

// One evaluation on the group's observations sObs [16][od] that wave 0 left in LDS: the single float32 product with obs_scale into sX
// (columns od .. XS - 1 and the rows beyond `rows` stay zero), then forward().  Starts with the caller's LDS in order (a workgroup
// barrier behind the writes of sObs).
template <int IN, int OU, class A>
__device__ __forceinline__ float stage(const A& a, int rows, long g, const float* sObs, float* smem, const Lane& L,
                                       const float (&w2)[128], const SmallRegs<IN, OU>& r, float& zmax, bool& saw_nan) {
    constexpr int XSW = xs_of<IN>();
    const int od = obs_dim_of(a);
    float* sX = smem + A_IMG;
    if (threadIdx.x < GROUP * XSW) {
        const int row = threadIdx.x / XSW, i = threadIdx.x % XSW;
        float xv = 0.f;
        if (g * GROUP + row < rows && i < od) xv = sObs[row * od + i] * a.scale[i];
        saw_nan |= xv != xv;
        sX[threadIdx.x] = xv;
    }
    return forward<IN, OU>(smem, L, w2, r, zmax);
}
// (the output partials forward() left: out_preact's operand)
template <int IN>
__device__ __forceinline__ const float* part_of(const float* smem) { return smem + A_IMG + GROUP * xs_of<IN>(); }

template <class A>
__device__ __forceinline__ void report(const A& a, float zmax, bool saw_nan) {
    report_activation_range(a.status, zmax);
    if (a.status && saw_nan) atomicOr(a.status, MPG_STATUS_NAN);
}
}  // namespace policy_pass
