// The host-side step size of every Adam in the library: the native step driver's networks (train_step.cpp) and the learned temperature
// (optim_kernels.hip: mpg_sac_alpha_update).  mpg_amd/policy.py states the same operations.
#pragma once
#include <algorithm>
#include <cmath>

// PolynomialDecay (policy.py:54,62) and the ApplyAdam step size AS TENSORFLOW FORMS THEM: every operand a float32 tensor
// (schedule in the dtype of the initial rate; beta^t = pow of the float32 hyper-parameter; alpha = lr sqrt(1 - b2^t) / (1 - b1^t)
// in float32).  float32(0.999) is 1.3e-8 above 0.999, which puts alpha 6.7e-6 below the real-number formula for the first
// thousands of steps - found in round 6 when the reference's own PolicyWithQs.apply_gradients first ran against this path.
// beta^t: double-precision pow of the float32 operand rounded once = the correctly rounded powf.
inline float polynomial_decay(const float* sched, long long step) {
    const float lr0 = sched[0], S = sched[1], lr_end = sched[2];
    const float p = std::min((float)step, S) / S;
    return (lr0 - lr_end) * (1.f - p) + lr_end;
}

inline float adam_step_size(const float* sched, long long steps_done) {
    const float lr = polynomial_decay(sched, steps_done);
    const double t = (double)(steps_done + 1);
    const float b1p = (float)std::pow((double)0.9f, t), b2p = (float)std::pow((double)0.999f, t);
    return lr * std::sqrt(1.f - b2p) / (1.f - b1p);
}
