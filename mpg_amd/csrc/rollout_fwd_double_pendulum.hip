// The double-pendulum instantiations of the forward sweep (and the small kernel that writes their first-layer inputs for the
// weight-gradient launch) as their own translation unit (see the note in rollout_fwd.hip).
#define MPG_FWD_DOUBLE_PENDULUM_PART 1
#include "rollout_fwd.hip"
