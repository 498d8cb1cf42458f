"""`bench.py` in its plain form (no --full): the headline line alone, and `--dump-outputs DIR` with what the last timed step
left for its caller."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ('params', 'targets', 'adam_m', 'adam_v', 'grad', 'stats', 'grad_norms', 'worker_obs')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(600)
@pytest.mark.parametrize('nproc', [1, 2])
def test_plain_bench_line_and_dumped_outputs(nproc, tmp_path):
    """one GPU as the driver runs it, and two ranks time-sharing the one GPU of the test box (gloo, torch.distributed.run)"""
    env = dict(os.environ, MPG_BENCH_BURN_IN='60')
    bench = [os.path.join(ROOT, 'bench.py'), '--gpus', str(nproc), '--steps', '10', '--warmup', '3', '--dump-outputs', str(tmp_path)]
    if nproc == 1:
        cmd = [sys.executable] + bench
    else:
        env.update(MPG_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1',
               '--master-port', str(_free_port())] + bench
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=550)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'].startswith('env-steps/sec') and d['unit'] == 'env-steps/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32-via-split-f16' and d['n_gpus'] == nproc and d['steps'] == 10 and d['warmup'] == 3
    assert d['ms_per_step'] > 0
    np.testing.assert_allclose(d['value'], nproc * 4096 / (d['ms_per_step'] * 1e-3), rtol=1e-6)
    # lean: none of the --full measurements
    assert not {'roofline', 'cpu_baseline', 'side_configs', 'region_ms_per_step', 'exchange_forms_ms'} & set(d)
    got = {n: np.load(str(tmp_path / (n + '.npy'))) for n in DUMPED}
    assert sorted(os.listdir(str(tmp_path))) == sorted(n + '.npy' for n in DUMPED)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    n = got['params'].size
    assert got['targets'].size == got['adam_m'].size == got['adam_v'].size == got['grad'].size == n
    assert got['worker_obs'].shape == (4096, 6) and got['grad_norms'].shape == (3,)
    assert not np.array_equal(got['params'], got['targets']) and np.abs(got['grad']).sum() > 0
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
