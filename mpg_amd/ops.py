"""Thin typed wrappers over the C ABI (include/mpg_hip.h).  Tensors in, tensors out; no arithmetic here."""
import ctypes

import torch

from . import _lib as L

ACT_LINEAR, ACT_TANH = 0, 1
STATUS_ACTIVATION_RANGE, STATUS_PARAMETER_RANGE, STATUS_NAN = 1, 2, 4      # MPG_STATUS_* (include/mpg_hip.h, "Numerical envelope")
HIDDEN = 256


class WCacheStruct(ctypes.Structure):
    """mpg_wcache_t: caller-owned descriptor of the packed W2 images of one flat parameter vector"""
    _fields_ = [('params', ctypes.c_void_p), ('packed', ctypes.c_void_p), ('n_nets', ctypes.c_int),
                ('in_dim', ctypes.c_int * 8), ('out_dim', ctypes.c_int * 8), ('status', ctypes.c_void_p)]


class CfgStruct(ctypes.Structure):
    """mpg_cfg_t"""
    _fields_ = [('obs_dim', ctypes.c_int), ('act_dim', ctypes.c_int), ('policy_out_act', ctypes.c_int),
                ('action_range', ctypes.c_float), ('obs_scale', ctypes.c_float * 16),
                ('rew_scale', ctypes.c_float), ('rew_shift', ctypes.c_float), ('gamma', ctypes.c_float),
                ('env_kind', ctypes.c_int),
                ('wcache', ctypes.POINTER(WCacheStruct) * 2), ('prof', ctypes.c_void_p), ('status', ctypes.c_void_p),
                ('grad_opts', ctypes.c_void_p)]      # mpg_grad_opts_t*: set by the native step driver only (NULL here)


class WeightCache(object):
    """Owns the packed images of one flat [net0 | net1 | ...] tensor (mpg_wcache_t + the device array).  Keep the object
    alive for as long as a cfg points at it; call pack() after writing `params` by anything but the Adam entry points."""

    def __init__(self, params, dims, status=None):
        k = len(dims)
        self.params = params
        self.status = status           # int32[1] device tensor the (re)packing reports MPG_STATUS_* bits into (keeps it alive)
        self.packed = torch.empty(L.lib().mpg_weight_cache_floats(L.c_int(k)), dtype=torch.float32, device=params.device)
        self.desc = WCacheStruct()
        self.desc.params, self.desc.packed, self.desc.n_nets = params.data_ptr(), self.packed.data_ptr(), k
        self.desc.status = status.data_ptr() if status is not None else None
        for i, (ind, outd) in enumerate(dims):
            self.desc.in_dim[i], self.desc.out_dim[i] = ind, outd
        self.pack()

    def pack(self):
        L.call('mpg_weight_cache_pack', ctypes.byref(self.desc), L.stream())

    @property
    def ref(self):
        return ctypes.byref(self.desc)

    @property
    def pointer(self):
        return ctypes.pointer(self.desc)


def _wc(cache):
    return cache.ref if cache is not None else None


class Profiler(object):
    """mpg_prof_t: caller-owned kernel timer; attach() makes the calls issued with that cfg report to it."""

    def __init__(self, max_samples=4096):
        self.h = ctypes.c_void_p(0)
        self._attached = []          # every cfg that carries this handle: cleared in close(), so none is left dangling
        L.call('mpg_prof_create', L.c_int(max_samples), ctypes.byref(self.h))

    def attach(self, *cfgs):
        for c in cfgs:
            c.prof = self.h.value
            if not any(c is a for a in self._attached):
                self._attached.append(c)

    def detach(self, *cfgs):
        for c in cfgs:
            if c.prof == self.h.value:
                c.prof = None
            self._attached = [a for a in self._attached if a is not c]

    def start(self, every):
        L.call('mpg_prof_start', self.h, L.c_int(every))

    def stop(self):
        L.call('mpg_prof_start', self.h, L.c_int(0))

    def read(self, slot):
        """(average ms per timed launch or None, number of timed launches)"""
        ms, cnt = ctypes.c_double(0), ctypes.c_int(0)
        L.call('mpg_prof_read', self.h, L.c_int(slot), ctypes.byref(ms), ctypes.byref(cnt))
        return (ms.value / cnt.value if cnt.value else None), cnt.value

    def close(self):
        if self.h:
            for c in self._attached:      # a cfg must never outlive the events it points at
                if c.prof == self.h.value:
                    c.prof = None
            self._attached = []
            L.lib().mpg_prof_destroy(self.h)
            self.h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_cfg(env_id='PathTracking-v0', obs_scale=None, rew_scale=None, rew_shift=0.0, gamma=0.98,
             policy_out_activation=None, action_range=None, obs_dim=None):
    """Defaults are the reference's (train_script.py:202-306 / train_script4mujoco.py:296-411).  obs_dim: 6 + num_future_data
    for PathTracking (train_script.py:794-811), up to 16 (num_future_data <= 10, the env's own limit here)."""
    pt = env_id == 'PathTracking-v0'
    if env_id == DOUBLE_PENDULUM:
        return _double_pendulum_cfg(obs_scale, rew_scale, rew_shift, gamma, policy_out_activation, action_range)
    c = CfgStruct()
    c.obs_dim, c.act_dim = (int(obs_dim) if (pt and obs_dim) else 6, 2) if pt else (4, 1)
    if pt and not 6 <= c.obs_dim <= 16:
        # the library's own answer for such a cfg is MPG_EINVAL at the first launch (net_cfg_ok, csrc/host_glue.h): raise it where the cfg is built
        raise L.MpgError('MPG_EINVAL: PathTracking observations have 6 + num_future_data entries and the env and network kernels serve '
                         'num_future_data <= 10 (policy inputs up to 16 wide, critic inputs up to 18; got obs_dim %d)' % c.obs_dim)
    if policy_out_activation is None:
        policy_out_activation = 'tanh' if pt else 'linear'
    c.policy_out_act = ACT_TANH if policy_out_activation == 'tanh' else ACT_LINEAR
    if action_range is None:
        action_range = 0.0 if pt else 3.0
    c.action_range = float(action_range or 0.0)
    sc = obs_scale if obs_scale is not None else ([1., 1., 2., 1., 2.4, 1 / 1200] if pt else [0.001, 1 / 3, 0.1, 0.5])
    for i in range(16):
        c.obs_scale[i] = float(sc[i]) if i < len(sc) else 1.0
    c.rew_scale = float(rew_scale if rew_scale is not None else (0.01 if pt else 1.0))
    c.rew_shift = float(rew_shift)
    c.gamma = float(gamma)
    c.env_kind = 0 if pt else 1
    return c


DOUBLE_PENDULUM = 'InvertedDoublePendulum-v2'


def _double_pendulum_cfg(obs_scale, rew_scale, rew_shift, gamma, policy_out_activation, action_range):
    """The reference registers the model (envs_and_models/__init__.py:12-15) but ships no parser for this env, so the defaults are this
    project's choice: unit observation scale, reward scale 1, linear policy output with action_range 1.0 - a = tanh(mean), the
    model's own "think of actions are in range [-1, 1]" (inverted_double_pendulum_model.py:134).  Observation: the env's 11 entries
    [p, sin t1, sin t2, cos t1, cos t2, pdot, t1dot, t2dot, frc x 3] (:105); one action."""
    c = CfgStruct()
    c.obs_dim, c.act_dim = 11, 1
    c.policy_out_act = ACT_TANH if (policy_out_activation or 'linear') == 'tanh' else ACT_LINEAR
    c.action_range = float((1.0 if action_range is None else action_range) or 0.0)
    sc = obs_scale if obs_scale is not None else [1.] * 11
    for i in range(16):
        c.obs_scale[i] = float(sc[i]) if i < len(sc) else 1.0
    c.rew_scale = float(rew_scale if rew_scale is not None else 1.0)
    c.rew_shift = float(rew_shift)
    c.gamma = float(gamma)
    c.env_kind = 2       # MPG_ENV_INVERTED_DOUBLE_PENDULUM
    return c


def net_size(in_dim, out_dim):
    return in_dim * HIDDEN + HIDDEN + HIDDEN * HIDDEN + HIDDEN + HIDDEN * out_dim + out_dim


def policy_size(cfg):
    return net_size(cfg.obs_dim, 2 * cfg.act_dim)


def q_size(cfg):
    return net_size(cfg.obs_dim + cfg.act_dim, 1)


class Workspace(object):
    """Caller-owned scratch the ABI asks for (grown on demand, reused across calls on one stream)."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=self.device)
        return self.buf


_WS = {}


def workspace(device, nbytes, slot=0):
    key = (str(device), slot)
    if key not in _WS:
        _WS[key] = Workspace(device)
    return _WS[key].get(nbytes)


def _ws(device, slot, query, cfg, *sizes):
    """The caller's half of the workspace contract: ask `query`, refuse what it refuses (0 bytes), hold that many bytes.
    Returns the (pointer, size) pair the entry point takes."""
    nb = getattr(L.lib(), query)(ctypes.byref(cfg), *[L.c_int(int(v)) for v in sizes])
    if nb == 0:
        raise L.MpgError('%s: unsupported configuration' % query)
    ws = workspace(device, nb, slot)
    return L.ptr(ws), L.c_size_t(ws.numel())


def _ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), (t.dtype, t.device, t.is_contiguous())
    return t


def mlp_forward(params, in_dim, out_dim, out_used, out_act, x, in_scale=None, n_scaled=0, wcache=None):
    rows = x.shape[0]
    y = torch.empty(rows, out_used, dtype=torch.float32, device=x.device)
    sc = (ctypes.c_float * 16)(*([float(v) for v in in_scale] + [1.0] * (16 - len(in_scale)))) if in_scale is not None else None
    L.call('mpg_mlp_forward', L.ptr(_f32(params)), L.c_int(in_dim), L.c_int(out_dim), L.c_int(out_used),
           L.c_int(out_act), L.c_int(rows), L.ptr(_f32(x)), sc, L.c_int(n_scaled), L.ptr(y), _wc(wcache), L.stream())
    return y


def policy_action(cfg, policy_params, obs, explore_sigma=0.0, seed=0, ctr=0):
    rows = obs.shape[0]
    act = torch.empty(rows, cfg.act_dim, dtype=torch.float32, device=obs.device)
    L.call('mpg_policy_action', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(rows), L.ptr(_f32(obs)),
           L.c_float(explore_sigma), L.c_u64(seed), L.c_u64(ctr), L.ptr(act), L.stream())
    return act


def q_targets(cfg, policy_t, q1t, q2t, rew, obs_tp1, smooth_eps=None, smooth_sigma=0.2, smooth_clip=0.5):
    rows = obs_tp1.shape[0]
    y = torch.empty(rows, dtype=torch.float32, device=obs_tp1.device)
    ws = _ws(obs_tp1.device, 0, 'mpg_q_targets_workspace_bytes', cfg, rows)
    L.call('mpg_q_targets', ctypes.byref(cfg), L.ptr(_f32(policy_t)), L.ptr(_f32(q1t)),
           L.ptr(_f32(q2t) if q2t is not None else None), L.c_int(rows), L.ptr(_f32(rew)), L.ptr(_f32(obs_tp1)),
           L.ptr(_f32(smooth_eps) if smooth_eps is not None else None), L.c_float(smooth_sigma),
           L.c_float(smooth_clip), L.ptr(y), *ws, L.stream())
    return y


def td3_targets(cfg, policy_t, q1t, q2t, rew, obs_tp1, smooth_eps, smooth_sigma=0.2, smooth_clip=0.5):
    """(y, y1): the smoothed clipped double-Q target and the plain Q1 target of the priorities' td error from ONE evaluation of
    the target policy (mpg_td3_targets; td3.py:69-92)."""
    rows = obs_tp1.shape[0]
    y = torch.empty(rows, dtype=torch.float32, device=obs_tp1.device)
    y1 = torch.empty(rows, dtype=torch.float32, device=obs_tp1.device)
    ws = _ws(obs_tp1.device, 0, 'mpg_q_targets_workspace_bytes', cfg, rows)
    L.call('mpg_td3_targets', ctypes.byref(cfg), L.ptr(_f32(policy_t)), L.ptr(_f32(q1t)), L.ptr(_f32(q2t)), L.c_int(rows),
           L.ptr(_f32(rew)), L.ptr(_f32(obs_tp1)), L.ptr(_f32(smooth_eps) if smooth_eps is not None else None),
           L.c_float(smooth_sigma), L.c_float(smooth_clip), L.ptr(y), L.ptr(y1), *ws, L.stream())
    return y, y1


def normal_fill(n, seed, ctr, device):
    """n standard normals from the library's Philox stream (mpg_normal_fill)"""
    out = torch.empty(n, dtype=torch.float32, device=device)
    L.call('mpg_normal_fill', L.c_int(n), L.c_u64(seed), L.c_u64(ctr), L.ptr(out), L.stream())
    return out


def td3_priority_errors(y1, y, td):
    """(y1 - y) - td  = y1 - Q1(s, a), the priorities' td error of TD3 (td3.py:83-92) from the critic pass's own td output"""
    out = torch.empty_like(td)
    L.call('mpg_td3_priority_errors', L.c_int(td.numel()), L.ptr(_f32(y1)), L.ptr(_f32(y)), L.ptr(_f32(td)), L.ptr(out), L.stream())
    return out


PENDULUM_NSTEP_Q_CLIP = (-0.5, 0.0)      # MPG_PENDULUM_NSTEP_Q_LO / _HI (include/mpg_hip.h; mpg_learner.py:163-164)


def nstep_targets(cfg, policy_t, q1t, rewards, last_obs, clip=None):
    """mpg_nstep_targets; with clip=(lo, hi) mpg_nstep_targets_clipped: the bootstrap value clipped to [lo, hi] first"""
    n, rows = rewards.shape
    y = torch.empty(rows, dtype=torch.float32, device=last_obs.device)
    ws = _ws(last_obs.device, 0, 'mpg_q_targets_workspace_bytes', cfg, rows)
    if clip is not None:
        L.call('mpg_nstep_targets_clipped', ctypes.byref(cfg), L.ptr(_f32(policy_t)), L.ptr(_f32(q1t)), L.c_int(rows), L.c_int(n),
               L.ptr(_f32(rewards)), L.ptr(_f32(last_obs)), L.c_float(clip[0]), L.c_float(clip[1]), L.ptr(y), *ws, L.stream())
        return y
    L.call('mpg_nstep_targets', ctypes.byref(cfg), L.ptr(_f32(policy_t)), L.ptr(_f32(q1t)), L.c_int(rows), L.c_int(n),
           L.ptr(_f32(rewards)), L.ptr(_f32(last_obs)), L.ptr(y), *ws, L.stream())
    return y


def env_rollout(cfg, policy_params, obs0, act0, n, entry=None):
    """mpg_env_rollout / mpg_env_rollout_pendulum (by cfg.env_kind): n real-env steps from (obs0 [rows, obs_dim], act0 [rows, act_dim]),
    later actions from the policy without noise, ONE launch.  Returns (rewards [n, rows] RAW, last_obs [rows, obs_dim])."""
    rows, dev = obs0.shape[0], obs0.device
    rewards = torch.empty(int(n), rows, dtype=torch.float32, device=dev)
    last_obs = torch.empty(rows, cfg.obs_dim, dtype=torch.float32, device=dev)
    L.call(entry or ('mpg_env_rollout_pendulum' if cfg.env_kind == 1 else 'mpg_env_rollout'), ctypes.byref(cfg), L.ptr(_f32(policy_params)),
           L.c_int(rows), L.c_int(int(n)), L.ptr(_f32(obs0)), L.ptr(_f32(act0)), L.ptr(rewards), L.ptr(last_obs), L.stream())
    return rewards, last_obs


def env_rollout_pendulum(cfg, policy_params, obs0, act0, n):
    """env_rollout through the pendulum's entry point whatever cfg says: another env's cfg is refused under that name, not served"""
    return env_rollout(cfg, policy_params, obs0, act0, n, entry='mpg_env_rollout_pendulum')


EVAL_METRICS_PATH_TRACKING, EVAL_METRICS_PENDULUM = 8, 18      # MPG_EVAL_METRICS_* (include/mpg_hip.h): metrics per episode
# the rows of eval_metrics, in the reference's key_list order (evaluator.py:161,180-181,202-205)
EVAL_METRIC_KEYS = {
    0: ('episode_return', 'episode_len', 'delta_y_mse', 'delta_phi_mse', 'delta_v_mse', 'stationary_rew_mean', 'steer_mse', 'acc_mse'),
    1: ('episode_return', 'episode_len', 'x_mean', 'x_var', 'theta_mean', 'theta_var', 'xdot_mean', 'xdot_var', 'thetadot_mean',
        'thetadot_var', 'x_mse', 'theta_mse', 'xdot_mse', 'thetadot_mse', 'x_mse_25', 'theta_mse_25', 'xdot_mse_25', 'thetadot_mse_25')}


def eval_rollout(cfg, policy_params, state, obs, steps):
    """mpg_eval_rollout / mpg_eval_rollout_pendulum (by cfg.env_kind): `steps` deterministic steps (policy_action without noise, then the
    env's step; `done` is not consulted, nothing is reset) from the env's state block [8, n] and its observations obs [n, obs_dim] in ONE
    launch, bit-identical to the 2 * steps launches it replaces.  `state` is advanced in place; `obs` is left as it is (the launch works
    on a copy, which comes back as last_obs).  Returns (obs_traj [steps, n, obs_dim] - the observations BEFORE each step -, act_traj
    [steps, n, act_dim], rew_traj [steps, n], last_obs [n, obs_dim], done [n] uint8 of the last step) and, on PathTracking,
    done_intended [n] behind them."""
    n, dev, steps = obs.shape[0], obs.device, int(steps)
    od, ad = cfg.obs_dim, cfg.act_dim
    assert obs.shape == (n, od) and state.shape == (8, n), (obs.shape, state.shape)
    obs_io = _f32(obs).clone()
    rows = max(steps, 0)
    obs_traj = torch.empty(rows, n, od, dtype=torch.float32, device=dev)
    act_traj = torch.empty(rows, n, ad, dtype=torch.float32, device=dev)
    rew_traj = torch.empty(rows, n, dtype=torch.float32, device=dev)
    done = torch.empty(n, dtype=torch.uint8, device=dev)
    if cfg.env_kind == 1:
        L.call('mpg_eval_rollout_pendulum', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.c_int(steps), L.ptr(_f32(state)),
               L.ptr(obs_io), L.ptr(obs_traj), L.ptr(act_traj), L.ptr(rew_traj), L.ptr(done), L.stream())
        return obs_traj, act_traj, rew_traj, obs_io, done
    done_intended = torch.empty(n, dtype=torch.uint8, device=dev)
    L.call('mpg_eval_rollout', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.c_int(steps), L.ptr(_f32(state)), L.ptr(obs_io),
           L.ptr(obs_traj), L.ptr(act_traj), L.ptr(rew_traj), L.ptr(done), L.ptr(done_intended), L.stream())
    return obs_traj, act_traj, rew_traj, obs_io, done, done_intended


def eval_metrics(env_kind, obs_traj, act_traj, rew_traj):
    """mpg_eval_metrics: the reference's per-episode metrics (evaluator.py:160-211; rows: EVAL_METRIC_KEYS[env_kind]) of the recorded
    trajectories [steps, n, .] and their means over the episodes, float64, in ONE launch.  Returns (per_episode [K, n], mean [K])."""
    n = obs_traj.shape[1]
    out = eval_metrics_flat(env_kind, obs_traj, act_traj, rew_traj)
    K = out.numel() // (n + 1)
    return out[:K * n].view(K, n), out[K * n:]


def eval_metrics_flat(env_kind, obs_traj, act_traj, rew_traj):
    """eval_metrics' two results as the ONE device array they are views of - [K * n | K] float64 - so that one copy brings both to the
    host"""
    steps, n, od = obs_traj.shape
    K = {0: EVAL_METRICS_PATH_TRACKING, 1: EVAL_METRICS_PENDULUM}.get(int(env_kind), 1)
    out = torch.empty(K * (n + 1), dtype=torch.float64, device=obs_traj.device)
    L.call('mpg_eval_metrics', L.c_int(int(env_kind)), L.c_int(n), L.c_int(steps), L.c_int(od), L.ptr(_f32(obs_traj)),
           L.ptr(_f32(act_traj)), L.ptr(_f32(rew_traj)), L.ptr(out[:K * n]), L.ptr(out[K * n:]), L.stream())
    return out


def _model_eps(eps, shape, name):
    if eps is None:
        return None
    if tuple(eps.shape) != shape:
        raise ValueError('%s: eps has shape %s, the model noise of this call is %s (or None for zeros)' % (name, tuple(eps.shape), shape))
    return _f32(eps)


def model_step(cfg, obs, act, eps=None):
    """mpg_model_step: ONE rollout_out of the differentiable model cfg.env_kind names (the double pendulum included) on obs [rows, obs_dim]
    and act [rows, act_dim]; eps [rows] standard-normal model noise, None = zeros.  Returns (obs_next [rows, obs_dim], rew [rows] RAW)."""
    rows, dev = obs.shape[0], obs.device
    if tuple(obs.shape) != (rows, cfg.obs_dim) or tuple(act.shape) != (rows, cfg.act_dim):
        raise ValueError('model_step: obs %s and act %s are not [rows, %d] and [rows, %d]'
                         % (tuple(obs.shape), tuple(act.shape), cfg.obs_dim, cfg.act_dim))
    eps = _model_eps(eps, (rows,), 'model_step')
    obs_next = torch.empty(rows, cfg.obs_dim, dtype=torch.float32, device=dev)
    rew = torch.empty(rows, dtype=torch.float32, device=dev)
    L.call('mpg_model_step', ctypes.byref(cfg), L.c_int(rows), L.ptr(_f32(obs)), L.ptr(_f32(act)), L.ptr(eps), L.ptr(obs_next), L.ptr(rew),
           L.stream())
    return obs_next, rew


def model_rollout(cfg, policy_params, obs0, steps, eps=None):
    """mpg_model_rollout: the policy's closed loop on the model from obs0 [n, obs_dim] - `steps` pairs of policy_action (no noise) and
    model_step - in ONE launch, bit-identical to that chain; eps [steps, n] standard-normal model noise, None = zeros.  Returns (obs_traj
    [steps, n, obs_dim] - the observations BEFORE each step -, act_traj [steps, n, act_dim], rew_traj [steps, n] RAW, last_obs
    [n, obs_dim]): eval_rollout's record."""
    n, dev, steps = obs0.shape[0], obs0.device, int(steps)
    od, ad = cfg.obs_dim, cfg.act_dim
    if tuple(obs0.shape) != (n, od):
        raise ValueError('model_rollout: obs0 %s is not [n, %d]' % (tuple(obs0.shape), od))
    eps = _model_eps(eps, (steps, n), 'model_rollout')
    rows = max(steps, 0)
    obs_traj = torch.empty(rows, n, od, dtype=torch.float32, device=dev)
    act_traj = torch.empty(rows, n, ad, dtype=torch.float32, device=dev)
    rew_traj = torch.empty(rows, n, dtype=torch.float32, device=dev)
    last_obs = torch.empty(n, od, dtype=torch.float32, device=dev)
    L.call('mpg_model_rollout', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.c_int(steps), L.ptr(_f32(obs0)), L.ptr(eps),
           L.ptr(obs_traj), L.ptr(act_traj), L.ptr(rew_traj), L.ptr(last_obs), L.stream())
    return obs_traj, act_traj, rew_traj, last_obs


def _i32(t):
    assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous(), (t.dtype, t.device, t.is_contiguous())
    return t


def _model_env_rows(name, cfg, obs, age, act=None):
    n = obs.shape[0]
    if tuple(obs.shape) != (n, cfg.obs_dim) or tuple(age.shape) != (n,) or (act is not None and tuple(act.shape) != (n, cfg.act_dim)):
        raise ValueError('%s: obs %s, age %s%s are not [n, %d], [n]%s' % (
            name, tuple(obs.shape), tuple(age.shape), '' if act is None else ' and act %s' % (tuple(act.shape),), cfg.obs_dim,
            '' if act is None else ' and [n, %d]' % cfg.act_dim))
    return n


def model_env_reset(cfg, obs_io, age_io, seed, ctr, done_mask=None):
    """mpg_model_env_reset: re-draws the agents of the model-backed env (env_kind 2) whose done_mask byte is not 0 (None: all) in place -
    obs_io [n, 11], age_io [n] int32 - keyed (seed, ctr); the others are left untouched."""
    n = _model_env_rows('model_env_reset', cfg, obs_io, age_io)
    assert done_mask is None or (done_mask.dtype == torch.uint8 and tuple(done_mask.shape) == (n,))
    L.call('mpg_model_env_reset', ctypes.byref(cfg), L.c_int(n), L.ptr(_f32(obs_io)), L.ptr(_i32(age_io)), L.ptr(done_mask), L.c_u64(seed),
           L.c_u64(ctr), L.stream())


def model_env_step(cfg, obs, act, age_io, max_steps=0):
    """mpg_model_env_step: one step of the model-backed env - model_step's (obs_next, RAW rew) and done [n] uint8 = fell | truncated
    (age + 1 >= max_steps > 0); age_io [n] int32 is advanced in place.  Returns (obs_next, rew, done)."""
    n, dev = _model_env_rows('model_env_step', cfg, obs, age_io, act), obs.device
    obs_next = torch.empty(n, cfg.obs_dim, dtype=torch.float32, device=dev)
    rew = torch.empty(n, dtype=torch.float32, device=dev)
    done = torch.empty(n, dtype=torch.uint8, device=dev)
    L.call('mpg_model_env_step', ctypes.byref(cfg), L.c_int(n), L.ptr(_f32(obs)), L.ptr(_f32(act)), L.c_int(int(max_steps)),
           L.ptr(_i32(age_io)), L.ptr(obs_next), L.ptr(rew), L.ptr(done), L.stream())
    return obs_next, rew, done


def model_env_step_store_reset(cfg, obs_io, act, age_io, max_steps, ring, capacity, next_idx, seed, ctr, done_out=None):
    """mpg_model_env_step_store_reset: model_env_step, the transition into ring = (obs, act, rew, obs2, done) at (next_idx + i) % capacity
    and model_env_reset of the done agents keyed (seed, ctr) in ONE launch, bit-identical to the three calls; obs_io and age_io are
    advanced in place."""
    n = _model_env_rows('model_env_step_store_reset', cfg, obs_io, age_io, act)
    r_obs, r_act, r_rew, r_obs2, r_done = ring
    assert r_done.dtype == torch.uint8 and (done_out is None or done_out.dtype == torch.uint8)
    L.call('mpg_model_env_step_store_reset', ctypes.byref(cfg), L.c_int(n), L.ptr(_f32(obs_io)), L.ptr(_f32(act)), L.c_int(int(max_steps)),
           L.ptr(_i32(age_io)), L.c_int(int(capacity)), L.c_int(int(next_idx)), L.ptr(_f32(r_obs)), L.ptr(_f32(r_act)), L.ptr(_f32(r_rew)),
           L.ptr(_f32(r_obs2)), L.ptr(r_done), L.c_u64(seed), L.c_u64(ctr), L.ptr(done_out), L.stream())


def q_loss_grad(cfg, q_params, obs, act, y, inv_b_global=None, grad_out=None, loss_out=None, want_td=False):
    rows = obs.shape[0]
    dev = obs.device
    grad = grad_out if grad_out is not None else torch.empty(q_size(cfg), dtype=torch.float32, device=dev)
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=dev)
    td = torch.empty(rows, dtype=torch.float32, device=dev) if want_td else None
    ws = _ws(dev, 0, 'mpg_q_loss_grad_workspace_bytes', cfg, rows)
    L.call('mpg_q_loss_grad', ctypes.byref(cfg), L.ptr(_f32(q_params)), L.c_int(rows), L.ptr(_f32(obs)),
           L.ptr(_f32(act)), L.ptr(_f32(y)), L.c_float(inv_b_global if inv_b_global is not None else 1.0 / rows),
           L.ptr(loss), L.ptr(grad), L.ptr(td), *ws, L.stream())
    return loss, grad, td


def rollout_pg(cfg, policy_params, q1_params, obs0, eps, select, w, M=1, inv_b_global=None, all_steps_param_grad=False,
               grad_out=None, stats_out=None, n=None, noise_seed=0, noise_ctr=0):
    """mpg_rollout_pg: n-step model rollout + (mixed) policy gradient.  Returns (ret_sum, ret_sqsum, grad).
    eps=None draws the model noise inside the kernel (Philox(noise_seed, noise_ctr)); then pass n."""
    rows = obs0.shape[0]
    if eps is not None:
        n = eps.shape[0]
        assert eps.shape[1] == rows * M
    dev = obs0.device
    ns = len(select)
    grad = grad_out if grad_out is not None else torch.empty(policy_size(cfg), dtype=torch.float32, device=dev)
    stats = stats_out if stats_out is not None else torch.empty(2 * ns, dtype=torch.float32, device=dev)
    sel = _ints(select)
    wv = _floats(w)
    ws = _ws(dev, 1, 'mpg_rollout_pg_workspace_bytes', cfg, rows, M, n, ns, all_steps_param_grad)
    L.call('mpg_rollout_pg', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.ptr(_f32(q1_params)), L.c_int(rows),
           L.c_int(M), L.c_int(n), sel, L.c_int(ns), wv, L.ptr(_f32(obs0)), L.ptr(_f32(eps) if eps is not None else None),
           L.c_u64(noise_seed), L.c_u64(noise_ctr), L.c_float(inv_b_global if inv_b_global is not None else 1.0 / rows), L.c_int(int(all_steps_param_grad)),
           L.ptr(stats[:ns]), L.ptr(stats[ns:]), L.ptr(grad), *ws, L.stream())
    return stats[:ns], stats[ns:], grad


def ampc_pg(cfg, policy_params, obs0, eps, M=1, inv_b_global=None, grad_out=None, stats_out=None, n=None, noise_seed=0, noise_ctr=0):
    """mpg_ampc_pg: n-step model rollout without a critic, every step through the policy, no discount.  Returns (ret_sum [1],
    ret_sqsum [1], grad).  eps=None draws the model noise inside the kernel (Philox(noise_seed, noise_ctr)); then pass n."""
    rows, dev = obs0.shape[0], obs0.device
    if eps is not None:
        n = eps.shape[0]
        assert eps.shape[1] == rows * M
    grad = grad_out if grad_out is not None else torch.empty(policy_size(cfg), dtype=torch.float32, device=dev)
    stats = stats_out if stats_out is not None else torch.empty(2, dtype=torch.float32, device=dev)
    ws = _ws(dev, 1, 'mpg_ampc_pg_workspace_bytes', cfg, rows, M, n)
    L.call('mpg_ampc_pg', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(rows), L.c_int(M), L.c_int(n), L.ptr(_f32(obs0)),
           L.ptr(_f32(eps) if eps is not None else None), L.c_u64(noise_seed), L.c_u64(noise_ctr),
           L.c_float(inv_b_global if inv_b_global is not None else 1.0 / rows), L.ptr(stats[0:1]), L.ptr(stats[1:2]), L.ptr(grad), *ws,
           L.stream())
    return stats[0:1], stats[1:2], grad


CLIP_PARTS = 272          # MPG_CLIP_PARTS (include/mpg_hip.h)


def sq_partials(grad, seg_sizes, sq_part=None):
    ns = len(seg_sizes)
    part = sq_part if sq_part is not None else torch.empty(ns * CLIP_PARTS, dtype=torch.float32, device=grad.device)
    segs = _ints(seg_sizes)
    L.call('mpg_sq_partials', L.ptr(_f32(grad)), segs, L.c_int(ns), L.ptr(part), L.stream())
    return part


def clip_adam_polyak(w, m, v, target, grad, sq_part, seg_sizes, clip, lr_t, do_adam, do_polyak, tau, norms, nonfinite=None,
                     wc_w=None, wc_target=None):
    """mpg_clip_adam_polyak: second half of the clip + Adam + Polyak in one launch"""
    ns = len(seg_sizes)
    segs = _ints(seg_sizes)
    lr = _floats(lr_t)
    da = _ints(do_adam)
    dp = _ints(do_polyak)
    L.call('mpg_clip_adam_polyak', L.ptr(_f32(w)), L.ptr(_f32(m)), L.ptr(_f32(v)), L.ptr(target), L.ptr(_f32(grad)),
           L.ptr(_f32(sq_part)), segs, L.c_int(ns), L.c_float(clip), lr, da, dp, L.c_float(tau), L.ptr(norms), L.ptr(nonfinite),
           _wc(wc_w), _wc(wc_target), L.stream())


def clip_by_global_norm(grad, seg_sizes, clip, norms_out=None, nonfinite=None, scratch=None):
    ns = len(seg_sizes)
    norms = norms_out if norms_out is not None else torch.empty(ns, dtype=torch.float32, device=grad.device)
    segs = _ints(seg_sizes)
    L.call('mpg_clip_by_global_norm', L.ptr(_f32(grad)), segs, L.c_int(ns), L.c_float(clip), L.ptr(norms),
           L.ptr(nonfinite), L.ptr(scratch), L.stream())
    return norms


def adam_polyak(w, m, v, target, grad, seg_sizes, lr_t, do_adam, do_polyak, tau, skip_flag=None, wc_w=None, wc_target=None):
    ns = len(seg_sizes)
    segs = _ints(seg_sizes)
    lr = _floats(lr_t)
    da = _ints(do_adam)
    dp = _ints(do_polyak)
    L.call('mpg_adam_polyak', L.ptr(_f32(w)), L.ptr(_f32(m)), L.ptr(_f32(v)), L.ptr(target), L.ptr(_f32(grad)), segs,
           L.c_int(ns), lr, da, dp, L.c_float(tau), L.ptr(skip_flag),
           L.c_int(skip_flag.numel() if skip_flag is not None else 0), _wc(wc_w), _wc(wc_target), L.stream())


def rollout_q_target(cfg, policy_params, q1t, obs0, act0, eps, n=None, noise_seed=0, noise_ctr=0):
    rows = obs0.shape[0]
    n = eps.shape[0] if eps is not None else n
    y = torch.empty(rows, dtype=torch.float32, device=obs0.device)
    ws = _ws(obs0.device, 0, 'mpg_rollout_q_target_workspace_bytes', cfg, rows)
    L.call('mpg_rollout_q_target', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.ptr(_f32(q1t)), L.c_int(rows), L.c_int(n),
           L.ptr(_f32(obs0)), L.ptr(_f32(act0)), L.ptr(_f32(eps) if eps is not None else None), L.c_u64(noise_seed),
           L.c_u64(noise_ctr), L.ptr(y), *ws, L.stream())
    return y


def rollout_q_estimation(cfg, policy_params, q1t, obs0, act0, eps, select, M=1, noise_seed=0, noise_ctr=0):
    """mpg_rollout_q_estimation -> [n_select * rows] (the reference's concatenation of the selected slices)"""
    rows, ns = obs0.shape[0], len(select)
    y = torch.empty(ns * rows, dtype=torch.float32, device=obs0.device)
    sel = _ints(select)
    ws = _ws(obs0.device, 0, 'mpg_rollout_q_estimation_workspace_bytes', cfg, rows, M, ns)
    L.call('mpg_rollout_q_estimation', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.ptr(_f32(q1t)), L.c_int(rows), L.c_int(M),
           sel, L.c_int(ns), L.ptr(_f32(obs0)), L.ptr(_f32(act0)), L.ptr(_f32(eps) if eps is not None else None),
           L.c_u64(noise_seed), L.c_u64(noise_ctr), L.ptr(y), *ws, L.stream())
    return y


def _policy_grad(name, cfg, policy_params, critics, obs, extra, n_stats, inv_b_global, grad_out, stats_out, more_out=()):
    """the mpg_*_policy_grad call: (cfg, policy, critics..., rows, obs, extra..., inv_b, one pointer per statistic, more_out..., grad,
    workspace); more_out: further one-float outputs (None: allocated here), returned behind (stats, grad)"""
    rows, dev = obs.shape[0], obs.device
    more_out = tuple(t if t is not None else torch.empty(1, dtype=torch.float32, device=dev) for t in more_out)
    grad = grad_out if grad_out is not None else torch.empty(policy_size(cfg), dtype=torch.float32, device=dev)
    stats = stats_out if stats_out is not None else torch.empty(n_stats, dtype=torch.float32, device=dev)
    ws = _ws(dev, 1, name.replace('_auto', '') + '_workspace_bytes', cfg, rows)      # (an _auto form: its fixed-alpha sibling's query)
    L.call(name, ctypes.byref(cfg), L.ptr(_f32(policy_params)), *[L.ptr(_f32(q)) for q in critics], L.c_int(rows), L.ptr(_f32(obs)), *extra,
           L.c_float(inv_b_global if inv_b_global is not None else 1.0 / rows), *[L.ptr(stats[i:i + 1]) for i in range(n_stats)],
           *[L.ptr(t) for t in more_out], L.ptr(grad), *ws, L.stream())
    return (stats, grad) + more_out


def td3_policy_grad(cfg, policy_params, q1, q2, obs, inv_b_global=None, grad_out=None, stats_out=None):
    return _policy_grad('mpg_td3_policy_grad', cfg, policy_params, (q1, q2), obs, (), 2, inv_b_global, grad_out, stats_out)


def dpg_policy_grad(cfg, policy_params, q1, obs, inv_b_global=None, grad_out=None, stats_out=None):
    """mpg_dpg_policy_grad: -mean Q1(s~, pi(s~)) and its policy gradient.  Returns (stats = [q_sum, q_sqsum], grad)."""
    return _policy_grad('mpg_dpg_policy_grad', cfg, policy_params, (q1,), obs, (), 2, inv_b_global, grad_out, stats_out)


# ---- SAC's stochastic head, one body per call: on the plain Gaussian head or - the mpg_*_squashed entry points, include/mpg_hip.h "SAC with
# an action range": R = cfg.action_range > 0, PathTracking (act_dim 2) or the inverted pendulum (act_dim 1) - the tanh-squashed one
def _policy_sample(entry, cfg, policy_params, obs, eps, want_logits):
    rows, dev = obs.shape[0], obs.device
    act = torch.empty(rows, cfg.act_dim, dtype=torch.float32, device=dev)
    logp = torch.empty(rows, dtype=torch.float32, device=dev)
    logits = torch.empty(rows, 2 * cfg.act_dim, dtype=torch.float32, device=dev) if want_logits else None
    ws = _ws(dev, 0, entry + '_workspace_bytes', cfg, rows)
    L.call(entry, ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(rows), L.ptr(_f32(obs)), L.ptr(_f32(eps)),
           L.ptr(act), L.ptr(logp), L.ptr(logits), *ws, L.stream())
    return (act, logp, logits) if want_logits else (act, logp)


def policy_sample(cfg, policy_params, obs, eps, want_logits=False):
    """mpg_policy_sample: (act, logp[, logits]) of the Gaussian policy on the caller's standard-normal draws eps [rows, act_dim]
    (PolicyWithQs.compute_action, stochastic branch, policy.py:200-204)"""
    return _policy_sample('mpg_policy_sample', cfg, policy_params, obs, eps, want_logits)


def policy_sample_squashed(cfg, policy_params, obs, eps, want_logits=False):
    """mpg_policy_sample_squashed: act = R tanh(mean + sigma eps), logp with the bijectors' correction[, the plain logits]"""
    return _policy_sample('mpg_policy_sample_squashed', cfg, policy_params, obs, eps, want_logits)


def worker_sample_step(cfg, policy_params, state, obs_io, sample_seed, sample_ctr, ring, capacity, next_idx, env_seed, env_ctr,
                       want_logp=True, done_out=None):
    """mpg_worker_sample_step: OffPolicyWorker.sample's inner body for a stochastic policy in ONE launch - the draw
    (mpg_normal_fill(2 n, sample_seed, sample_ctr)), mpg_policy_sample and mpg_env_step_store_reset.  obs_io [n, obs_dim] holds the
    current observations and receives the next ones; ring = (obs, act, rew, obs2, done) arrays of `capacity` rows, written at
    (next_idx + i) % capacity.  Returns (act [n, 2], logp [n] or None)."""
    n, dev = obs_io.shape[0], obs_io.device
    act = torch.empty(n, cfg.act_dim, dtype=torch.float32, device=dev)
    logp = torch.empty(n, dtype=torch.float32, device=dev) if want_logp else None
    r_obs, r_act, r_rew, r_obs2, r_done = ring
    assert r_done.dtype == torch.uint8 and (done_out is None or done_out.dtype == torch.uint8)
    L.call('mpg_worker_sample_step', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.ptr(_f32(state)), L.ptr(_f32(obs_io)),
           L.c_u64(sample_seed), L.c_u64(sample_ctr), L.ptr(act), L.ptr(logp), L.c_int(int(capacity)), L.c_int(int(next_idx)),
           L.ptr(_f32(r_obs)), L.ptr(_f32(r_act)), L.ptr(_f32(r_rew)), L.ptr(_f32(r_obs2)), L.ptr(r_done), L.c_u64(env_seed),
           L.c_u64(env_ctr), L.ptr(done_out), L.stream())
    return act, logp


def worker_rollout(cfg, policy_params, iters, state, obs_io, explore_sigma, noise_seed, noise_ctr, ring, capacity, next_idx, env_seed,
                   env_ctr, done_out=None, max_steps=0):
    """mpg_worker_rollout: `iters` iterations of OffPolicyWorker.sample's loop for a deterministic policy (policy -> + N(0, sigma) ->
    env.step -> ring -> env.reset) in ONE launch, bit-identical to `iters` mpg_worker_step calls with the counters advancing by one and
    the ring position by n.  state [8, n] and obs_io [n, obs_dim] are advanced in place; ring = (obs, act, rew, obs2, done) arrays of
    `capacity` >= iters * n rows, iteration `it` writes the slots (next_idx + it * n + i) % capacity; done_out [n] (optional) receives
    the last iteration's done flags.  Returns the last iteration's actions [n, 2].
    A pendulum cfg (env_kind 1: obs_dim 4, actions [n, 1]) goes to mpg_worker_rollout_pendulum, the same contract against `iters`
    pairs of mpg_policy_action + mpg_env_step_store_reset.
    A double-pendulum cfg (env_kind 2: obs_dim 11, actions [n, 1]) goes to mpg_worker_rollout_model, the sample on the model-backed env:
    `state` is the agents' step counts [n] int32, max_steps the episode limit (0: none; read by this kind only), the contract the same
    against `iters` pairs of mpg_policy_action + mpg_model_env_step_store_reset."""
    n, dev = obs_io.shape[0], obs_io.device
    act = torch.empty(n, cfg.act_dim, dtype=torch.float32, device=dev)
    r_obs, r_act, r_rew, r_obs2, r_done = ring
    assert r_done.dtype == torch.uint8 and (done_out is None or done_out.dtype == torch.uint8)
    if cfg.env_kind == 2:
        L.call('mpg_worker_rollout_model', ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.c_int(int(iters)), L.ptr(_f32(obs_io)),
               L.ptr(_i32(state)), L.c_int(int(max_steps)), L.c_float(explore_sigma), L.c_u64(noise_seed), L.c_u64(noise_ctr), L.ptr(act),
               L.c_int(int(capacity)), L.c_int(int(next_idx)), L.ptr(_f32(r_obs)), L.ptr(_f32(r_act)), L.ptr(_f32(r_rew)), L.ptr(_f32(r_obs2)),
               L.ptr(r_done), L.c_u64(env_seed), L.c_u64(env_ctr), L.ptr(done_out), L.stream())
        return act
    entry = 'mpg_worker_rollout_pendulum' if cfg.env_kind == 1 else 'mpg_worker_rollout'
    L.call(entry, ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.c_int(int(iters)), L.ptr(_f32(state)),
           L.ptr(_f32(obs_io)), L.c_float(explore_sigma), L.c_u64(noise_seed), L.c_u64(noise_ctr), L.ptr(act), L.c_int(int(capacity)),
           L.c_int(int(next_idx)), L.ptr(_f32(r_obs)), L.ptr(_f32(r_act)), L.ptr(_f32(r_rew)), L.ptr(_f32(r_obs2)), L.ptr(r_done),
           L.c_u64(env_seed), L.c_u64(env_ctr), L.ptr(done_out), L.stream())
    return act


def worker_sample_rollout(cfg, policy_params, iters, state, obs_io, sample_seed, sample_ctr, ring, capacity, next_idx, env_seed, env_ctr,
                          done_out=None):
    """`iters` iterations of OffPolicyWorker.sample's loop for a stochastic policy (draw -> sample -> env.step -> ring -> env.reset) in
    ONE launch, bit-identical to `iters` triples of mpg_normal_fill(n * act_dim, sample_seed, sample_ctr + it), mpg_policy_sample[_squashed]
    and mpg_env_step_store_reset.  worker_rollout's arguments without explore_sigma; no log-density is returned.
    A PathTracking cfg (env_kind 0) goes to mpg_worker_sample_rollout: the Gaussian head, or with cfg.action_range > 0 the tanh-squashed
    one (a = range * tanh(mean + sigma * eps)); returns the last iteration's actions [n, 2].  Any other cfg goes to
    mpg_worker_sample_rollout_pendulum (the squashed head on the pendulum, actions [n, 1])."""
    n, dev = obs_io.shape[0], obs_io.device
    act = torch.empty(n, cfg.act_dim, dtype=torch.float32, device=dev)
    r_obs, r_act, r_rew, r_obs2, r_done = ring
    assert r_done.dtype == torch.uint8 and (done_out is None or done_out.dtype == torch.uint8)
    entry = 'mpg_worker_sample_rollout' if cfg.env_kind == 0 else 'mpg_worker_sample_rollout_pendulum'
    L.call(entry, ctypes.byref(cfg), L.ptr(_f32(policy_params)), L.c_int(n), L.c_int(int(iters)),
           L.ptr(_f32(state)), L.ptr(_f32(obs_io)), L.c_u64(sample_seed), L.c_u64(sample_ctr), L.ptr(act), L.c_int(int(capacity)),
           L.c_int(int(next_idx)), L.ptr(_f32(r_obs)), L.ptr(_f32(r_act)), L.ptr(_f32(r_rew)), L.ptr(_f32(r_obs2)), L.ptr(r_done),
           L.c_u64(env_seed), L.c_u64(env_ctr), L.ptr(done_out), L.stream())
    return act


def _sac_targets(entry, cfg, policy, q1t, q2t, rew, obs_tp1, eps, temp):
    rows = obs_tp1.shape[0]          # (temp: the entry point's temperature argument - alpha as a c_float, or the pointer to log_alpha)
    y = torch.empty(rows, dtype=torch.float32, device=obs_tp1.device)
    ws = _ws(obs_tp1.device, 0, entry.replace('_auto', '') + '_workspace_bytes', cfg, rows)
    L.call(entry, ctypes.byref(cfg), L.ptr(_f32(policy)), L.ptr(_f32(q1t)), L.ptr(_f32(q2t)), L.c_int(rows), L.ptr(_f32(rew)),
           L.ptr(_f32(obs_tp1)), L.ptr(_f32(eps)), temp, L.ptr(y), *ws, L.stream())
    return y


def sac_targets(cfg, policy, q1t, q2t, rew, obs_tp1, eps, alpha):
    """mpg_sac_targets: y = (rew + shift) * scale + gamma * (min(Q1t, Q2t)(s', a') - alpha * logp'), (a', logp') sampled from
    `policy` - the ONLINE one in the reference, sac.py:71 - with eps"""
    return _sac_targets('mpg_sac_targets', cfg, policy, q1t, q2t, rew, obs_tp1, eps, L.c_float(alpha))


def sac_targets_squashed(cfg, policy, q1t, q2t, rew, obs_tp1, eps, alpha):
    return _sac_targets('mpg_sac_targets_squashed', cfg, policy, q1t, q2t, rew, obs_tp1, eps, L.c_float(alpha))


def sac_targets_auto(cfg, policy, q1t, q2t, rew, obs_tp1, eps, log_alpha):
    """mpg_sac_targets_auto: mpg_sac_targets with alpha = exp(log_alpha[0]) read on the device (log_alpha: device tensor)"""
    return _sac_targets('mpg_sac_targets_auto', cfg, policy, q1t, q2t, rew, obs_tp1, eps, L.ptr(_f32(log_alpha)))


def sac_targets_squashed_auto(cfg, policy, q1t, q2t, rew, obs_tp1, eps, log_alpha):
    return _sac_targets('mpg_sac_targets_squashed_auto', cfg, policy, q1t, q2t, rew, obs_tp1, eps, L.ptr(_f32(log_alpha)))


def sac_policy_grad(cfg, policy_params, q1, q2, obs, eps, alpha, inv_b_global=None, grad_out=None, stats_out=None):
    """mpg_sac_policy_grad: mean(alpha * logp - min Q) and its policy gradient over all four output columns.
    Returns (stats = [qmin_sum, qmin_sqsum, logp_sum], grad)."""
    return _policy_grad('mpg_sac_policy_grad', cfg, policy_params, (q1, q2), obs, (L.ptr(_f32(eps)), L.c_float(alpha)), 3, inv_b_global,
                        grad_out, stats_out)


def sac_policy_grad_squashed(cfg, policy_params, q1, q2, obs, eps, alpha, inv_b_global=None, grad_out=None, stats_out=None):
    return _policy_grad('mpg_sac_policy_grad_squashed', cfg, policy_params, (q1, q2), obs, (L.ptr(_f32(eps)), L.c_float(alpha)), 3,
                        inv_b_global, grad_out, stats_out)


def sac_policy_grad_auto(cfg, policy_params, q1, q2, obs, eps, log_alpha, eps_alpha, target_entropy, inv_b_global=None, grad_out=None,
                         stats_out=None, alpha_grad_out=None):
    """mpg_sac_policy_grad_auto: mpg_sac_policy_grad with the device temperature, and this process's share of the temperature's
    gradient -inv_b * sum(logp(eps_alpha) + target_entropy) from the same pass.  Returns (stats = [qmin_sum, qmin_sqsum, logp_sum],
    grad, alpha_grad [1])."""
    return _policy_grad('mpg_sac_policy_grad_auto', cfg, policy_params, (q1, q2), obs,
                        (L.ptr(_f32(eps)), L.ptr(_f32(log_alpha)), L.ptr(_f32(eps_alpha)), L.c_float(target_entropy)), 3, inv_b_global, grad_out,
                        stats_out, (alpha_grad_out,))


def sac_policy_grad_squashed_auto(cfg, policy_params, q1, q2, obs, eps, log_alpha, eps_alpha, target_entropy, inv_b_global=None,
                                  grad_out=None, stats_out=None, alpha_grad_out=None):
    return _policy_grad('mpg_sac_policy_grad_squashed_auto', cfg, policy_params, (q1, q2), obs,
                        (L.ptr(_f32(eps)), L.ptr(_f32(log_alpha)), L.ptr(_f32(eps_alpha)), L.c_float(target_entropy)), 3, inv_b_global, grad_out,
                        stats_out, (alpha_grad_out,))


class SacAlphaStruct(ctypes.Structure):
    """mpg_sac_alpha_t: the learned temperature of SAC - its device state block (8 floats: log_alpha, Adam m, Adam v, then the snapshot
    of the last gradient call: alpha, alpha_loss, |g|, non-finite flag, 0), target_entropy, its Adam's schedule and step counter"""
    _fields_ = [('state', ctypes.c_void_p), ('target_entropy', ctypes.c_float), ('lr', ctypes.c_float * 3),
                ('opt_steps', ctypes.c_longlong)]


ALPHA_STATE_FLOATS = 8
ALPHA_LOG, ALPHA_M, ALPHA_V, ALPHA_SNAPSHOT, ALPHA_LOSS, ALPHA_NORM, ALPHA_NONFINITE = range(7)      # slots of the state block


def sac_alpha_update(desc, g, clip=1.0, do_clip=False, do_adam=False, skip_flag=None):
    """mpg_sac_alpha_update on the SacAlphaStruct `desc`: the clip of the reduced gradient g [1] (with the statistics' snapshot) and /
    or one Adam step of log_alpha; desc.opt_steps advances with do_adam"""
    L.call('mpg_sac_alpha_update', ctypes.byref(desc), L.ptr(_f32(g)), L.c_float(clip), L.c_int(int(do_clip)), L.c_int(int(do_adam)),
           L.ptr(skip_flag), L.c_int(skip_flag.numel() if skip_flag is not None else 0), L.stream())


def mpg_gradients_supported(cfg, rows, M, n, n_select, n_q):
    """whether mpg_mpg_gradients serves these sizes: its workspace query answers 0 for what the entry point refuses"""
    return L.lib().mpg_mpg_gradients_workspace_bytes(ctypes.byref(cfg), *[L.c_int(int(v)) for v in (rows, M, n, n_select, n_q)]) != 0


def mpg_gradients(cfg, n_q, params, target_params, obs, act, rew, obs_tp1, y_in, select, w, grad, stats, y_out, M=1, n=None,
                  eps=None, noise_seed=0, noise_ctr=0, inv_b_global=None, sq_part=None):
    """mpg_mpg_gradients: MPGLearner.compute_gradient without the clip (targets unless y_in, critic grads, mixed PG)."""
    rows, dev = obs.shape[0], obs.device
    if eps is not None:
        n = eps.shape[0]
    ns = len(select)
    sel = _ints(select)
    wv = _floats(w)
    ws = _ws(dev, 1, 'mpg_mpg_gradients_workspace_bytes', cfg, rows, M, n, ns, n_q)
    L.call('mpg_mpg_gradients', ctypes.byref(cfg), L.c_int(n_q), L.ptr(_f32(params)), L.ptr(target_params), L.c_int(rows),
           L.ptr(_f32(obs)), L.ptr(_f32(act)), L.ptr(rew), L.ptr(obs_tp1), L.ptr(y_in), L.c_int(M), L.c_int(n), sel,
           L.c_int(ns), wv, L.ptr(eps), L.c_u64(noise_seed), L.c_u64(noise_ctr),
           L.c_float(inv_b_global if inv_b_global is not None else 1.0 / rows), L.ptr(_f32(grad)), L.ptr(_f32(stats)),
           L.ptr(_f32(y_out)), L.ptr(sq_part), None, *ws, L.stream())
