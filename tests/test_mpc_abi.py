"""mpg_mpc_cost_grad and mpg_mpc_solve at the drop-in boundary, without a GPU: both libraries export them with the declared argument
types, and every refusal comes back as MPG_EINVAL with a text of its own before any launch, the outputs untouched (the buffers are
HOST arrays with a pattern in them: a launch would fault, a refusal never dereferences them)."""
import ctypes
import math
import os
import re

import pytest

from mpg_amd import _lib as L

COST, SOLVE = 'mpg_mpc_cost_grad', 'mpg_mpc_solve'
NULL = ctypes.c_void_p(0)
I, F = ctypes.c_int, ctypes.c_float
MPG_EINVAL = -1000
ENGINES = sorted(L.ENGINES)
ROOT = os.path.join(os.path.dirname(L.HEADER), '..')
SRC = os.path.join(ROOT, 'mpg_amd', 'csrc', 'mpc_kernels.hip')
PATTERN = 0x5A


@pytest.fixture(scope='module', autouse=True)
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_points(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    for name in (COST, SOLVE):
        assert name in L.declared_symbols()
        assert hasattr(lib, name)
        assert L.declared_return_types()[name] == 'int'
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed


def _declared(name):
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
    assert m, name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def test_declared_argument_types():
    assert _declared(COST) == ['int rows', 'int horizon', 'const float* x0', 'const float* u', 'float* cost', 'float* grad', 'float* traj',
                               'mpg_stream_t stream']
    assert _declared(SOLVE) == ['int rows', 'int horizon', 'int iters', 'float tol', 'const float* x0', 'float* u_io', 'float* cost_out',
                                'float* pgnorm_out', 'int* info', 'mpg_stream_t stream']


def test_every_constant_of_the_method_is_a_named_define_the_kernel_uses():
    hdr = open(L.HEADER).read()
    krn = open(SRC).read()
    want = {'MPG_MPC_MAX_HORIZON': '31', 'MPG_MPC_MAX_ITERS': '1000', 'MPG_MPC_STEER_SCALE': '0.4f', 'MPG_MPC_ACC_SCALE': '3.0f',
            'MPG_MPC_SPG_M': '5', 'MPG_MPC_SPG_HALVINGS': '20', 'MPG_MPC_SPG_GAMMA': '1e-4f', 'MPG_MPC_SPG_ALPHA0': '0.05f',
            'MPG_MPC_SPG_ALPHA_MAX_STEP': '10.0f', 'MPG_MPC_SPG_ALPHA_LO': '1e-6f', 'MPG_MPC_SPG_ALPHA_HI': '1e3f'}
    for name, value in want.items():
        assert re.findall(r'#define\s+%s\s+(\S+)' % name, hdr) == [value], name
        assert name in krn, name
    from mpg_amd import mpc
    assert (mpc.MAX_HORIZON, mpc.MAX_ITERS) == (31, 1000)


class Buffers(object):
    """host arrays behind every pointer argument, filled with a pattern"""

    def __init__(self):
        self.raw = {k: (ctypes.c_ubyte * 4096)(*([PATTERN] * 4096)) for k in ('x0', 'u', 'cost', 'grad', 'traj', 'pgnorm', 'info')}

    def p(self, k):
        return ctypes.cast(self.raw[k], ctypes.c_void_p)

    def untouched(self):
        return all(bytes(v) == bytes([PATTERN]) * 4096 for v in self.raw.values())


OK = dict(rows=3, horizon=25, iters=200, tol=0.)
SHARED = [(dict(rows=0), 'no rows'), (dict(rows=-2), 'no rows'), (dict(horizon=0), 'horizon >= 1'), (dict(horizon=-1), 'horizon >= 1'),
          (dict(horizon=32), 'horizon <= 31'), (dict(horizon=1 << 20), 'horizon <= 31')]
COST_REFUSALS = SHARED + [({k: None}, 'null pointer') for k in ('x0', 'u', 'cost')]
SOLVE_REFUSALS = SHARED + [(dict(iters=-1), 'iters >= 0'), (dict(iters=1001), 'iters <= 1000'), (dict(tol=-1e-3), 'tol negative or NaN'),
                           (dict(tol=math.nan), 'tol negative or NaN'), (dict(tol=-math.inf), 'tol negative or NaN')] + \
    [({k: None}, 'null pointer') for k in ('x0', 'u', 'cost', 'pgnorm', 'info')]


def _call(lib, name, a, buf):
    def p(k):
        return NULL if (k in a and a[k] is None) else buf.p(k)
    if name == COST:
        return lib.mpg_mpc_cost_grad(I(a['rows']), I(a['horizon']), p('x0'), p('u'), p('cost'), p('grad'), p('traj'), NULL)
    return lib.mpg_mpc_solve(I(a['rows']), I(a['horizon']), I(a['iters']), F(a['tol']), p('x0'), p('u'), p('cost'), p('pgnorm'), p('info'),
                             NULL)


def _ids(table):
    return ['%02d-%s' % (i, re.sub(r'[^a-z0-9]+', '_', c[1].lower())) for i, c in enumerate(table)]


def _refused(engine, name, case):
    diff, text = case
    with L.engine(engine):
        lib = L.lib()
        a = dict(OK)
        a.update(diff)
        buf = Buffers()
        rc = _call(lib, name, a, buf)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith(name + ':') and text in msg, msg
        assert buf.untouched()


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(COST_REFUSALS)), ids=_ids(COST_REFUSALS))
def test_cost_grad_refusals(engine, case):
    _refused(engine, COST, COST_REFUSALS[case])


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(SOLVE_REFUSALS)), ids=_ids(SOLVE_REFUSALS))
def test_solve_refusals(engine, case):
    _refused(engine, SOLVE, SOLVE_REFUSALS[case])


def test_the_first_thing_wrong_answers():
    """several things wrong at once: the refusals come in the order of the header's list"""
    lib = L.lib()
    buf = Buffers()
    assert _call(lib, SOLVE, dict(rows=0, horizon=40, iters=-1, tol=-1.), buf) == MPG_EINVAL
    assert 'no rows' in lib.mpg_last_error().decode()
    assert _call(lib, SOLVE, dict(rows=1, horizon=40, iters=-1, tol=-1.), buf) == MPG_EINVAL
    assert 'horizon <= 31' in lib.mpg_last_error().decode()
    assert _call(lib, SOLVE, dict(rows=1, horizon=31, iters=1000, tol=-1., x0=None), buf) == MPG_EINVAL
    assert 'tol negative or NaN' in lib.mpg_last_error().decode()
    assert buf.untouched()


@pytest.mark.parametrize('name, least', [(COST, 4), (SOLVE, 7)])
def test_every_refusal_has_a_text_of_its_own(name, least):
    src = open(SRC).read()
    body = src[src.index('extern "C" int %s(' % name):]
    body = body[:body.index('hipLaunchKernelGGL')]
    texts = re.findall(r'MPG_REQUIRE\(.*?"(%s: [^"]*)"' % name, body, flags=re.S)
    assert len(texts) == least and len(set(texts)) == len(texts), texts


def test_a_refusal_reaches_python_as_mpg_error():
    """L.call - what mpg_amd.mpc sends its arguments through - turns a refusal into MpgError with the library's text; the wrappers
    themselves take device tensors (tests/test_mpc_gpu.py::test_wrappers_raise_mpg_error)"""
    buf = Buffers()
    with pytest.raises(L.MpgError, match=SOLVE + ': iters <= 1000'):
        L.call(SOLVE, I(4), I(25), I(1001), F(0.), buf.p('x0'), buf.p('u'), buf.p('cost'), buf.p('pgnorm'), buf.p('info'), NULL)
    with pytest.raises(L.MpgError, match=COST + ': horizon <= 31'):
        L.call(COST, I(4), I(32), buf.p('x0'), buf.p('u'), buf.p('cost'), NULL, NULL, NULL)
    assert buf.untouched()


def test_the_product_module_imports_nothing_from_the_oracle():
    src = open(os.path.join(ROOT, 'mpg_amd', 'mpc.py')).read()
    assert not re.search(r'^\s*(import|from)\s+(oracle|tests)\b', src, flags=re.M)
    assert 'mpc_oracle' not in src
    from mpg_amd import mpc
    for name in ('ModelPredictiveControl', 'run_mpc', 'mpc_cost_grad', 'mpc_solve'):
        assert callable(getattr(mpc, name))
    for name in ('reset_init_x', 'cost_function', 'cost_and_gradient', 'solve'):
        assert callable(getattr(mpc.ModelPredictiveControl, name))
