"""The tanh-squashed Gaussian head on the GPU, both engines: the (in 4, used-out 2) network pass against a float64 MLP; the
mpg_*_squashed entry points against float64 autograd of the restatement (tests/sac_tanh_oracle.py) with its float32 run as the
reference's own error, under tests/yardstick.py - on the inverted pendulum and on PathTracking with 0 and 3 look-ahead entries,
strided and packed weight images, the fixed and the device-read temperature (bit-identical to each other); saturated rows and clipped
log-std logits; the logits and the action's formation on PathTracking; two unequal shards; SACLearner on the fixtures of the
unmodified reference (tests/golden/make_golden_sac_tanh.py); the training loop on the pendulum; repeated launches."""
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from oracle import mpg_oracle as O
from tests import sac_tanh_oracle as T
from tests import yardstick as Y
from tests.golden_inputs import mlp_weights_flat, reset_law_obs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOG_ALPHA = np.float32(np.log(0.2))
# the temperature of every entry-point case: the fixed-alpha forms take it as a float, the _auto forms read log_alpha on the device
ALPHA = float(np.float32(np.exp(np.float64(LOG_ALPHA))))
TARGET_ENTROPY = -2.0
# name -> (env, look-ahead entries K, action range)
CONFS = {'pendulum': (T.PEND, 0, 3.0), 'pt': (T.PT, 0, 2.0), 'pt-K3': (T.PT, 3, 2.0)}
ROWS = (16, 40, 272, 8200)        # one row group; a partial one; 17 groups; 513 groups: the many-block sums and the two-group forward


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def host(t):
    return t.detach().cpu().numpy()


def sigma32(log_std):
    """exp(clip(log_std, -5, 1)) as the correctly rounded float32 value (include/mpg_hip.h)"""
    return torch.exp(torch.clamp(log_std, -5., 1.).double()).float()


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    with L.engine(request.param):
        yield request.param


# ---- 1: the (4, 2) forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [ops.ACT_LINEAR, ops.ACT_TANH], ids=['linear', 'tanh'])
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_four_by_two_forward(engine, cache, act):
    """both logits of the pendulum's policy against mpg_mlp_forward's float64 restatement (the bar of test_four_output_forward); the
    first column bit for bit the one-output pass"""
    rng = np.random.Generator(np.random.PCG64(404))
    flat = mlp_weights_flat(rng, 4, 2)
    scale = rng.uniform(0.5, 2.0, 4)
    ws = O.unflatten(flat, 4, 256, 2, dtype=torch.float64)
    params = dev(flat)
    wc = ops.WeightCache(params, [(4, 2)]) if cache else None
    for rows in (1, 16, 17, 40, 8200):
        x = rng.standard_normal((rows, 4)).astype(np.float32)
        y2 = ops.mlp_forward(params, 4, 2, 2, act, dev(x), in_scale=scale, n_scaled=4, wcache=wc)
        y1 = ops.mlp_forward(params, 4, 2, 1, act, dev(x), in_scale=scale, n_scaled=4, wcache=wc)
        assert y2.shape == (rows, 2)
        assert torch.equal(bits(y2[:, :1]), bits(y1)), (rows, 'the first column is the one-output pass')
        ref = O.mlp(ws, torch.as_tensor(x, dtype=torch.float64) * torch.as_tensor(scale.astype(np.float32)).double(),
                    'tanh' if act else 'linear').numpy()
        err = np.abs(host(y2) - ref).max()
        assert err <= 2e-5 * max(1.0, np.abs(ref).max()), (rows, err)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def conf_dims(conf):
    env, K, R = CONFS[conf]
    od, ad = T.dims(env, K)
    return env, K, R, od, ad


def draw_obs(rng, env, K, rows):
    if env == T.PEND:
        return (rng.standard_normal((rows, 4)) * np.array([0.5, 0.1, 0.5, 0.5])).astype(np.float32)
    return np.concatenate([reset_law_obs(rng, rows), rng.standard_normal((rows, K)).astype(np.float32)], 1)


def reference(c, dtype):
    """the restatement at `dtype` on the case's draws: logits, u, sample, log-density, soft target (the online networks stand in for
    the targets), the policy loss pieces, the UNCLIPPED policy gradient, the log-density under the third draw"""
    env, K, R, od, ad = conf_dims(c['conf'])
    cfg = T.make_cfg(env, R, K, alpha=ALPHA)
    cfg.gamma = c['gamma']
    nets = O.Nets(cfg, c['w'], dtype=dtype)
    t = lambda x: torch.as_tensor(x).to(dtype)
    po = O.process_obses(cfg, t(c['obs']))
    with torch.no_grad():
        logits = O.mlp(nets.w['policy'], po, 'linear')
        a, logp, u = T.head(cfg, logits, t(c['eps']))
        logp_alpha = T.head(cfg, logits, t(c['eps_alpha']))[1]
    y, _ = T.soft_target(cfg, nets, t(c['rew']), t(c['obs']), t(c['eps']))
    _, grads, _, _, _, _ = T.policy_forward_and_backward(cfg, nets, t(c['obs']), t(c['eps']))
    qmin = torch.minimum(nets.q('Q1', po, a), nets.q('Q2', po, a)).detach()
    return dict(logits=logits.numpy(), u=u.numpy(), a=a.numpy(), logp=logp.numpy(), y=y.numpy(), qmin=qmin.numpy(),
                grad=np.concatenate([g.numpy().ravel() for g in grads]), logp_alpha=logp_alpha.numpy())


def finish_case(c):
    c['r32'], c['r64'] = reference(c, torch.float32), reference(c, torch.float64)
    return c


@functools.lru_cache(maxsize=None)
def make_case(conf, rows, seed):
    """(computed once per set of arguments and shared by the engines / weight-image forms; nothing in it is written to later)"""
    env, K, R, od, ad = conf_dims(conf)
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {'policy': mlp_weights_flat(rng, od, 2 * ad), 'Q1': mlp_weights_flat(rng, od + ad, 1), 'Q2': mlp_weights_flat(rng, od + ad, 1)}
    return finish_case(dict(conf=conf, rows=rows, w=w, obs=draw_obs(rng, env, K, rows), eps=rng.standard_normal((rows, ad)).astype(np.float32),
                            eps_alpha=rng.standard_normal((rows, ad)).astype(np.float32),
                            rew=(-rng.uniform(0, 5, rows)).astype(np.float32), gamma=0.98))


QUARTER = 68


@functools.lru_cache(maxsize=None)
def saturated_case(conf):
    """4 x 68 rows chosen, by the float64 restatement, out of a pool of 16384 observations under a policy whose mean columns are scaled by 8
    and whose log-std columns by 30: [0, 68) with max_k |u_k| between 8 and 15; [68, 136) with EVERY log-std logit outside [-5, 1], both
    sides present; [136, 272) with |u| below 4 and every log-std logit inside"""
    env, K, R, od, ad = conf_dims(conf)
    rng = np.random.Generator(np.random.PCG64(808 + od))
    w = {'policy': mlp_weights_flat(rng, od, 2 * ad), 'Q1': mlp_weights_flat(rng, od + ad, 1), 'Q2': mlp_weights_flat(rng, od + ad, 1)}
    w3 = w['policy'][-(256 * 2 * ad + 2 * ad):-2 * ad].reshape(256, 2 * ad)            # a view: edits land in the flat vector
    w3[:, :ad] *= 8.0
    w3[:, ad:] *= 30.0
    pool = 16384
    cfg = T.make_cfg(env, R, K)
    obs, eps = draw_obs(rng, env, K, pool), rng.standard_normal((pool, ad)).astype(np.float32)
    if env == T.PEND:         # (observations of unit size AFTER the scaling, so that the logits vary over the pool as PathTracking's do)
        obs = (rng.standard_normal((pool, 4)) / np.array(cfg.obs_scale)).astype(np.float32)
    with torch.no_grad():
        logits = O.mlp(O.Nets(cfg, w, dtype=torch.float64).w['policy'], O.process_obses(cfg, torch.as_tensor(obs).double()), 'linear')
        u = T.head(cfg, logits, torch.as_tensor(eps).double())[2].abs().max(1).values.numpy()
    ls = logits[:, ad:].numpy()
    out, inside = ((ls > 1.05) | (ls < -5.05)).all(1), ((ls > -4.95) & (ls < 0.95)).all(1)
    big = np.flatnonzero((u >= 8) & (u <= 15))[:QUARTER]
    hi = np.flatnonzero(out & (ls > 1).any(1) & (u < 8))[:QUARTER // 2]
    lo = np.flatnonzero(out & (ls < -5).all(1) & (u < 8))[:QUARTER // 2]
    calm = np.flatnonzero(inside & (u < 4))[:2 * QUARTER]
    assert (len(big), len(hi), len(lo), len(calm)) == (QUARTER, QUARTER // 2, QUARTER // 2, 2 * QUARTER), (len(big), len(hi), len(lo), len(calm))
    pick = np.concatenate([big, hi, lo, calm])
    rows = len(pick)
    return finish_case(dict(conf=conf, rows=rows, w=w, obs=obs[pick], eps=eps[pick], eps_alpha=rng.standard_normal((rows, ad)).astype(np.float32),
                            rew=(-rng.uniform(0, 5, rows)).astype(np.float32), gamma=0.98))


def on_device(case, cache=False):
    """the case on the device: its own cfg and tensors (the shared case stays as it is)"""
    env, K, R, od, ad = conf_dims(case['conf'])
    c = dict(case)
    ocfg = T.make_cfg(env, R, K)
    c['cfg'] = ops.make_cfg(env, obs_dim=od, obs_scale=ocfg.obs_scale, policy_out_activation='linear', gamma=c['gamma'], action_range=R)
    c['wp'], c['wq1'], c['wq2'] = dev(c['w']['policy']), dev(c['w']['Q1']), dev(c['w']['Q2'])
    if cache:           # the packed-image instantiations: cfg.wcache[0] -> the images of the three networks, one flat vector
        flat = torch.cat([c['wq1'], c['wq2'], c['wp']]).contiguous()
        nq = c['wq1'].numel()
        c['wq1'], c['wq2'], c['wp'] = flat[:nq], flat[nq:2 * nq], flat[2 * nq:]
        c['wc'] = ops.WeightCache(flat, [(od + ad, 1), (od + ad, 1), (od, 2 * ad)])
        c['cfg'].wcache[0] = c['wc'].pointer
    c['d'] = dict(obs=dev(c['obs']), eps=dev(c['eps']), eps_alpha=dev(c['eps_alpha']), rew=dev(c['rew']), log_alpha=dev(np.array([LOG_ALPHA])))
    c['nets'] = [('policy', od, 2 * ad)]
    return c


def check_arrays(got, r32, r64, nets, where):
    """every array of the flat policy gradient: error against float64 at most 4 x the float32 restatement's own + FLOOR"""
    worst, o = 0.0, 0
    for _, din, dout in nets:
        for shp in O.mlp_shapes(din, 256, dout):
            n = int(np.prod(shp))
            e_ref, e_got = Y.rel_l2(r32[o:o + n], r64[o:o + n]), Y.rel_l2(got[o:o + n], r64[o:o + n])
            allow = 4.0 * e_ref + Y.FLOOR
            print('%s %s: got %.2e, float32 restatement %.2e, allowance %.2e' % (where, shp, e_got, e_ref, allow))
            assert e_got <= allow, (where, shp, e_got, e_ref)
            worst = max(worst, e_got / allow)
            o += n
    assert o == got.size == r32.size == r64.size
    return worst


def alpha_grad_check(ag, r64, rows, inv_b, where):
    """-inv_b * sum(logp_alpha + target_entropy) against its float64 value, within the standard bound of a float32 sum of `rows` terms
    plus the terms' own float32 error (2e-6 relative: tests/test_sac_tanh_golden.py pins the density's at 2e-7)"""
    terms = r64['logp_alpha'].astype(np.float64) + TARGET_ENTROPY
    want, bound = -inv_b * terms.sum(), (rows * 2.0 ** -24 + 2e-6) * np.abs(terms).sum() * inv_b
    print('%s: alpha_grad %.7g, float64 %.7g, error %.2e, bound %.2e' % (where, ag, want, abs(ag - want), bound))
    assert abs(ag - want) <= bound, (where, ag, want, bound)


def run_entry_points(c, where):
    """every squashed entry point once on the case; returns (act, logp, logits, y, stats, grad, alpha_grad) after the checks that hold
    for any case: the range, the _auto forms bit for bit the fixed-alpha ones, values and gradients under the yardstick"""
    d, cfg, R = c['d'], c['cfg'], CONFS[c['conf']][2]
    r32, r64, rows = c['r32'], c['r64'], c['rows']
    act, logp, logits = ops.policy_sample_squashed(cfg, c['wp'], d['obs'], d['eps'], want_logits=True)
    assert act.abs().max().item() <= R and torch.isfinite(logp).all()
    print('%s: logp vs float64 %.2e (float32 restatement %.2e)' % (where, Y.rel_l2(host(logp), r64['logp']), Y.rel_l2(r32['logp'], r64['logp'])))
    Y.check_values(host(logp), r32['logp'], r64['logp'], what='logp ' + where)
    Y.check_values(host(act), r32['a'], r64['a'], what='act ' + where)
    a2, lp2 = ops.policy_sample_squashed(cfg, c['wp'], d['obs'], d['eps'])          # without logits_out: the workspace's own block
    assert torch.equal(bits(a2), bits(act)) and torch.equal(bits(lp2), bits(logp))
    q = (cfg, c['wp'], c['wq1'], c['wq2'])
    y = ops.sac_targets_squashed(*q, d['rew'], d['obs'], d['eps'], ALPHA)
    y_auto = ops.sac_targets_squashed_auto(*q, d['rew'], d['obs'], d['eps'], d['log_alpha'])
    assert torch.equal(bits(y_auto), bits(y)), where
    print('%s: targets got %.2e, float32 restatement %.2e' % (where, Y.rel_l2(host(y), r64['y']), Y.rel_l2(r32['y'], r64['y'])))
    Y.check_values(host(y), r32['y'], r64['y'], what='soft targets ' + where)
    stats, grad = ops.sac_policy_grad_squashed(*q, d['obs'], d['eps'], ALPHA)
    s_auto, g_auto, ag = ops.sac_policy_grad_squashed_auto(*q, d['obs'], d['eps'], d['log_alpha'], d['eps_alpha'], TARGET_ENTROPY)
    assert torch.equal(bits(g_auto), bits(grad)) and torch.equal(bits(s_auto), bits(stats)), where
    check_arrays(host(grad), r32['grad'], r64['grad'], c['nets'], where)
    s = host(stats).astype(np.float64)
    np.testing.assert_allclose(s[0], r64['qmin'].sum(), rtol=2e-5, atol=2e-5 * rows)         # the bars of tests/test_sac_gpu.py
    np.testing.assert_allclose(s[1], (r64['qmin'] ** 2).sum(), rtol=1e-4, atol=1e-6 * rows)
    np.testing.assert_allclose(s[2], r64['logp'].sum(), rtol=2e-5, atol=2e-5 * rows)
    alpha_grad_check(ag.item(), r64, rows, 1.0 / rows, where)
    return act, logp, logits, y, stats, grad, ag


# ---- 2: the entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conf', sorted(CONFS))
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_entry_points_vs_float64_autograd(engine, cache, rows, conf):
    c = on_device(make_case(conf, rows, 1600 + rows), cache)
    run_entry_points(c, '%s rows %d %s (%s)' % (conf, rows, 'packed' if cache else 'strided', engine))
    # alpha is READ on the device: another log_alpha, another alpha term, without a new call argument
    d, q = c['d'], (c['cfg'], c['wp'], c['wq1'], c['wq2'])
    d['log_alpha'].fill_(0.0)
    y_one = ops.sac_targets_squashed_auto(*q, d['rew'], d['obs'], d['eps'], d['log_alpha'])
    assert torch.equal(bits(y_one), bits(ops.sac_targets_squashed(*q, d['rew'], d['obs'], d['eps'], 1.0)))
    # the same draw and target_entropy 0: the temperature's sum is logp_sum's tree, finished as -inv_b * sum
    stats, _, ag = ops.sac_policy_grad_squashed_auto(*q, d['obs'], d['eps'], d['log_alpha'], d['eps'], 0.0)
    assert torch.equal(bits(ag), bits(-torch.tensor(1.0 / rows, dtype=torch.float32, device=DEV) * stats[2:3]))


# ---- 3: saturation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conf', sorted(CONFS))
def test_saturated_rows_and_clipped_log_std(engine, conf):
    env, K, R, od, ad = conf_dims(conf)
    c = on_device(saturated_case(conf))
    u, ls = np.abs(c['r64']['u']).max(1), c['r64']['logits'][:, ad:]
    assert ((u[:QUARTER] >= 8) & (u[:QUARTER] <= 15)).all()
    clipped = slice(QUARTER, 2 * QUARTER)
    assert ((ls[clipped] > 1) | (ls[clipped] < -5)).all() and (ls[clipped] > 1).any() and (ls[clipped] < -5).any()
    act, logp, logits, _, _, grad, _ = run_entry_points(c, 'saturated %s (%s)' % (conf, engine))
    assert act.abs().max().item() <= R and act[:QUARTER].abs().max(1).values.min().item() > R * (1 - 1e-6)
    assert torch.isfinite(logp).all() and torch.isfinite(grad).all()
    assert logp[:QUARTER].max().item() > 10.0                   # the bijector's correction at |u| >= 8: -log(1 - tanh^2) >= 14.6
    # the clipped quarter as a batch of its own: the log-std columns of the output layer receive EXACT zeros
    d, rows = c['d'], QUARTER
    sub = lambda t: t[clipped].clone()
    q = (c['cfg'], c['wp'], c['wq1'], c['wq2'])
    for g in (ops.sac_policy_grad_squashed(*q, sub(d['obs']), sub(d['eps']), ALPHA)[1],
              ops.sac_policy_grad_squashed_auto(*q, sub(d['obs']), sub(d['eps']), d['log_alpha'], sub(d['eps_alpha']), TARGET_ENTROPY)[1]):
        g = host(g)
        w3, b3 = g[-(256 * 2 * ad + 2 * ad):-2 * ad].reshape(256, 2 * ad), g[-2 * ad:]
        assert not w3[:, ad:].any() and not b3[ad:].any(), 'a clipped log-std logit has no gradient'
        assert np.abs(w3[:, :ad]).max() > 0 and np.abs(b3[:ad]).max() > 0 and np.isfinite(g).all()


# ---- 4: the logits and the action's formation --------------------------------------------------------------------------------
@pytest.mark.parametrize('conf', sorted(CONFS))
def test_the_range_never_reaches_the_logits(engine, conf):
    """PathTracking: logits_out is bit for bit mpg_policy_sample's on the same weights under a cfg without a range.  Every
    configuration: act within 1e-6 of R tanh(mean + sigma eps) formed from logits_out (u in float32 as the kernel forms it - product
    and sum rounded separately -, the tanh in float64)"""
    env, K, R, od, ad = conf_dims(conf)
    for rows in (40, 8200):
        c = on_device(make_case(conf, rows, 1600 + rows))
        d = c['d']
        act, logp, logits = ops.policy_sample_squashed(c['cfg'], c['wp'], d['obs'], d['eps'], want_logits=True)
        if env == T.PT:
            plain = ops.make_cfg(obs_dim=od, obs_scale=T.make_cfg(env, R, K).obs_scale, policy_out_activation='linear', gamma=c['gamma'])
            a0, lp0, logits0 = ops.policy_sample(plain, c['wp'], d['obs'], d['eps'], want_logits=True)
            assert torch.equal(bits(logits), bits(logits0))
            assert not torch.equal(bits(act), bits(a0)) and not torch.equal(bits(logp), bits(lp0))
        u32 = logits[:, :ad] + sigma32(logits[:, ad:]) * d['eps']
        formed = R * torch.tanh(u32.double())
        err = (act.double() - formed).abs().max().item()
        print('%s rows %d: |act - R tanh(u)| max %.2e' % (conf, rows, err))
        assert err <= 1e-6
        mode = ops.policy_action(c['cfg'], c['wp'], d['obs'])                        # compute_mode is unchanged: R tanh(mean)
        assert (mode.double() - R * torch.tanh(logits[:, :ad].double())).abs().max().item() <= 1e-6


# ---- 5: repeated launches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conf', ['pendulum', 'pt'])
def test_hundred_launches_are_bit_identical(engine, conf):
    for rows in (272, 8200):
        c = on_device(make_case(conf, rows, 1600 + rows))
        d, q = c['d'], (c['cfg'], c['wp'], c['wq1'], c['wq2'])
        grad_args = q + (d['obs'], d['eps'], d['log_alpha'], d['eps_alpha'], TARGET_ENTROPY)
        keep = [t.clone() for t in ops.sac_policy_grad_squashed_auto(*grad_args)]
        keep += [t.clone() for t in ops.policy_sample_squashed(c['cfg'], c['wp'], d['obs'], d['eps'])]
        keep.append(ops.sac_targets_squashed(*q, d['rew'], d['obs'], d['eps'], ALPHA).clone())
        for _ in range(100):
            got = list(ops.sac_policy_grad_squashed_auto(*grad_args)) + list(ops.policy_sample_squashed(c['cfg'], c['wp'], d['obs'], d['eps']))
            got.append(ops.sac_targets_squashed(*q, d['rew'], d['obs'], d['eps'], ALPHA))
            for a, b in zip(got, keep):
                assert torch.equal(bits(a), bits(b))


# ---- 6: data parallel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conf', sorted(CONFS))
def test_two_unequal_shards(engine, conf):
    """17 + 23 rows with inv_b_global = 1 / 40, in one process with the harness of tests/test_sharding_gpu.py: the shard partials of the
    policy gradient (fixed and device-read temperature) add up to float64 autograd's under the yardstick, the temperature's shares to
    the whole batch's, and inv_b_global scales exactly what carries it"""
    from tests import test_sharding_gpu as S
    B, cut = S.RAGGED
    c = on_device(make_case(conf, B, 1700))
    d, q, r32, r64 = c['d'], (c['cfg'], c['wp'], c['wq1'], c['wq2']), c['r32'], c['r64']

    def run(lo, hi, inv_b):
        stats, grad = ops.sac_policy_grad_squashed(*q, S.rows_of(d['obs'], lo, hi), S.rows_of(d['eps'], lo, hi), ALPHA, inv_b_global=inv_b)
        return dict(stats=stats, grad=grad)

    def run_auto(lo, hi, inv_b):
        stats, grad, ag = ops.sac_policy_grad_squashed_auto(*q, S.rows_of(d['obs'], lo, hi), S.rows_of(d['eps'], lo, hi), d['log_alpha'],
                                                            S.rows_of(d['eps_alpha'], lo, hi), TARGET_ENTROPY, inv_b_global=inv_b)
        return dict(stats=stats, grad=grad, alpha_grad=ag)
    for fn, scaled in ((run, ('grad',)), (run_auto, ('grad', 'alpha_grad'))):
        whole, parts = S.sharded(fn, B, cut)
        where = '%s B %d = %d + %d %s (%s)' % (fn.__name__, B, cut, B - cut, conf, engine)
        S.check_arrays(S.host(parts[0]['grad'] + parts[1]['grad']), S.host(whole['grad']), r32['grad'], r64['grad'], c['nets'], where)
        s = S.f64sum(parts, 'stats')
        np.testing.assert_allclose(s[0], r64['qmin'].sum(), rtol=2e-5, atol=2e-5 * B)
        np.testing.assert_allclose(s[1], (r64['qmin'] ** 2).sum(), rtol=1e-4, atol=1e-6 * B)
        np.testing.assert_allclose(s[2], r64['logp'].sum(), rtol=2e-5, atol=2e-5 * B)
        if 'alpha_grad' in whole:
            alpha_grad_check((parts[0]['alpha_grad'] + parts[1]['alpha_grad']).item(), r64, B, 1.0 / B, where + ' shares')
            alpha_grad_check(whole['alpha_grad'].item(), r64, B, 1.0 / B, where + ' unsharded')
        for lo, hi in ((0, cut), (cut, B)):
            S.check_scaling(fn, lo, hi, scaled, ('stats',), where)


# ---- 7: SACLearner against the fixtures of the unmodified reference -----------------------------------------------------------
BATCH_KEYS = ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')
FIXTURES = [('sac_tanh_pend_H256_B64.npz', T.PEND, False), ('sac_tanh_pend_auto_H256_B64.npz', T.PEND, True),
            ('sac_tanh_pt_H256_B64.npz', T.PT, False)]


def _learner(g, env, auto):
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    kw = dict(alpha='auto', target_entropy=float(g['target_entropy'])) if auto else {}
    args = default_args('SAC', env_id=env, replay_batch_size=64, gradient_clip_norm=T.CLIP, action_range=float(g['action_range']),
                        squashed_head=True, **kw)
    learner = SACLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    assert pw.names == ['Q1', 'Q2', 'policy'] and pw.squashed_head and pw.alpha == ('auto' if auto else T.ALPHA)
    w = T.fixture_weights(int(g['weights_seed']), env)
    flat = np.concatenate([w[n] for n in pw.names])
    pw.set_flat(flat, (flat * np.float32(g['target_scale'])).astype(np.float32))
    if auto:
        pw.log_alpha.fill_(float(g['log_alpha']))
    return learner


@pytest.mark.parametrize('name,env,auto', FIXTURES, ids=[f[0][:-4] for f in FIXTURES])
def test_compute_gradient_vs_reference_golden(golden, engine, name, env, auto):
    """the list the reference's SACLearner.compute_gradient returns under an action range, its targets, log-densities, actions and stats,
    on the same minibatch, weights and recorded draws"""
    g = golden(name)
    learner = _learner(g, env, auto)
    pw = learner.policy_with_value
    draws = dict(eps_target=dev(g['eps_target']), eps_policy=dev(g['eps_policy']), **(dict(eps_alpha=dev(g['eps_alpha'])) if auto else {}))
    grads = learner.compute_gradient([dev(g[k]) for k in BATCH_KEYS], None, None, 0, **draws)
    assert len(grads) == 18 + int(auto)
    got = host(torch.cat([x.reshape(-1) for x in grads[:18]]))
    where = '%s (%s)' % (name[:-4], engine)
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [(n,) + tuple(pw.dims[n]) for n in pw.names], where=where,
                              small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    Y.check_values(host(learner.batch_data['batch_targets']), g['targets'], g['targets_f64'], what='targets ' + where)
    pairs = [('target', 'batch_obs_tp1'), ('policy', 'batch_obs')] + ([('alpha', 'batch_obs')] if auto else [])
    for key, obs_key in pairs:                 # the head through the policy object, on every recorded draw
        act, logp = pw.compute_action(dev(g[obs_key]), dev(g['eps_' + key]))
        Y.check_values(host(logp), g['logp_' + key], g['logp_' + key + '_f64'], what='logp_' + key + ' ' + where)
        Y.check_values(host(act), g['act_' + key], g['act_' + key + '_f64'], what='act_' + key + ' ' + where)
        assert act.abs().max().item() <= float(g['action_range'])
    st = learner.get_stats()
    for k in ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'mb_targets_mean', 'value_mean', 'q_gradient_norm1', 'q_gradient_norm2',
              'policy_gradient_norm') + (('alpha', 'alpha_loss', 'alpha_gradient_norm') if auto else ()):
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)      # the tolerances of tests/test_sac_gpu.py
    assert max(st['q_gradient_norm1'], st['q_gradient_norm2']) > T.CLIP > st['policy_gradient_norm']
    if auto:
        Y.check_values(host(grads[18]), g['alpha_grad'], g['alpha_grad_f64'], what='temperature gradient ' + where)


# ---- 8: the loop on the pendulum ---------------------------------------------------------------------------------------------
SMALL = dict(interval=3, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256, max_buffer_size=1024)


def _stack(seed, auto, buffer_type='normal', **kw):
    from mpg_amd.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    interval = kw.pop('interval')
    extra = dict(alpha='auto', target_entropy=-1., delay_update=2) if auto else {}
    args = default_args('SAC', env_id=T.PEND, seed=seed, squashed_head=True, buffer_type=buffer_type, **extra, **kw)
    assert args.action_range == 3.0
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    rb = (ReplayBuffer if buffer_type == 'normal' else PrioritizedReplayBuffer)(args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=interval)
    assert opt._fused is None and worker.policy_with_value.squashed_head
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    if pw.auto_alpha:
        tensors.append(pw.alpha_state.clone())
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, pw._sample_ctr,
                opt.num_sampled_steps)
    return tensors, counters


@pytest.mark.parametrize('auto,buffer_type', [(False, 'normal'), (True, 'normal'), (False, 'priority')],
                         ids=['fixed-alpha', 'auto-alpha', 'fixed-alpha-prioritized'])
def test_pendulum_loop_is_finite_reproducible_and_resumes_bit_identically(tmp_path, engine, auto, buffer_type):
    """20 iterations of SingleProcessOffPolicyOptimizer with the squashed SACLearner on InvertedPendulumConti-v0: every parameter
    finite, every sampled action within [-3, 3]; a second run from the same seed is bit-identical; a checkpoint written at iteration 8
    and loaded into a stack built with ANOTHER seed ends bit-identical to the uninterrupted run"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint
    a = _stack(5, auto, buffer_type, **SMALL)
    for _ in range(8):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(12):
        a.step()
    ta, ca = _state(a)
    assert all(torch.isfinite(t).all() for t in ta[:4])
    assert ca[0] == ({'Q1': 20, 'Q2': 20, 'policy': 10} if auto else {'Q1': 20, 'Q2': 20, 'policy': 20})
    n = len(a.replay_buffer)
    acts = a.replay_buffer.act[:n]
    assert n >= 256 and acts.abs().max().item() <= 3.0 and acts.abs().max().item() > 0.0
    st = a.learner.get_stats()
    assert all(np.isfinite(st[k]) for k in ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'value_mean', 'value_var'))
    a.worker.policy_with_value.check_status()
    b = _stack(5, auto, buffer_type, **SMALL)
    for _ in range(20):
        b.step()
    tb, cb = _state(b)
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), i
    c = _stack(99, auto, buffer_type, **SMALL)                # different seed: every stream must come from the file
    meta = load_checkpoint(path, c)
    assert meta['optimizer']['iteration'] == 8 and c.iteration == 8 and meta['policy']['squashed_head'] is True
    for _ in range(12):
        c.step()
    tc, cc = _state(c)
    assert ca == cc, (ca, cc)
    for i, (x, y) in enumerate(zip(ta, tc)):
        assert torch.equal(x, y), i


def test_checkpoints_of_plain_and_squashed_heads_do_not_mix(tmp_path, engine):
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint, state_of
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker

    def pt_stack(**kw):
        small = dict(SMALL)
        interval = small.pop('interval')
        args = default_args('SAC', seed=5, **small, **kw)
        return SingleProcessOffPolicyOptimizer(OffPolicyWorker(PolicyWithQs, args.env_id, args, 0), SACLearner(PolicyWithQs, args),
                                               ReplayBuffer(args, 0), None, args, sampling_interval=interval)
    plain, squashed = pt_stack(), pt_stack(action_range=2.0, squashed_head=True)
    meta, _ = state_of(plain)
    assert 'squashed_head' not in meta['policy']                # a plain stack's file keeps its content
    with pytest.raises(ValueError, match='policy head'):
        load_checkpoint(save_checkpoint(str(tmp_path / 'plain.npz'), plain), squashed)
    with pytest.raises(ValueError, match='policy head'):
        load_checkpoint(save_checkpoint(str(tmp_path / 'squashed.npz'), squashed), plain)
    with pytest.raises(ValueError, match='native_sac=True: the tanh-squashed head'):
        SingleProcessOffPolicyOptimizer(squashed.worker, squashed.learner, squashed.replay_buffer, None, squashed.args, native_sac=True)
