// The double-pendulum instantiations of the reverse sweep as their own translation unit (see the note in rollout_bwd.hip).
#define MPG_BWD_DOUBLE_PENDULUM_PART 1
#include "rollout_bwd.hip"
