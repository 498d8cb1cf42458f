"""What the ABI tests of the one-launch rollouts share (tests/test_*_rollout*_abi.py; no GPU): the ctypes shorthands, the build fixture,
the refusal loop over a file's own REFUSALS table, the null-configuration check, and the ONE source-reading check that no two
conditions of an entry point share a text.  A test file keeps its table, its `_call` and its special cases."""
import ctypes
import os
import re

import pytest

from mpg_amd import _lib as L

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, U64 = ctypes.c_int, ctypes.c_float, ctypes.c_uint64
MPG_EINVAL = -1000
ENGINES = sorted(L.ENGINES)
CSRC = os.path.join(os.path.dirname(L.HEADER), '..', 'mpg_amd', 'csrc')


@pytest.fixture(scope='module', autouse=True)
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


def _with(c, **kw):
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def refused(engine, name, call, make, args, text):
    """call(lib, cfg_ref, args) on make()'s cfg is refused as MPG_EINVAL under the entry point's name with `text`"""
    with L.engine(engine):
        lib = L.lib()
        cfg = make()
        rc = call(lib, ctypes.byref(cfg), args)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith(name + ':') and text in msg, msg


def refusal_test(name, table, ok, call):
    """the test of a table of (cfg maker, what differs from `ok`, the text of the refusal), one case per row and engine"""
    @pytest.mark.parametrize('engine', ENGINES)
    @pytest.mark.parametrize('case', range(len(table)),
                             ids=['%02d-%s' % (i, re.sub(r'[^a-z0-9]+', '_', c[2].lower())) for i, c in enumerate(table)])
    def test(engine, case):
        make, diff, text = table[case]
        refused(engine, name, call, make, dict(ok, **diff), text)
    return test


def null_configuration_refused(engine, name, call, ok):
    with L.engine(engine):
        lib = L.lib()
        assert call(lib, NULL, dict(ok)) == MPG_EINVAL
        msg = lib.mpg_last_error().decode()
        assert msg.startswith(name + ':') and 'null configuration' in msg, msg


def _required(code, who):
    """the texts of the MPG_REQUIREs of `code` that begin with `who` (a name, or the helpers' '%s'), without it"""
    return [t[len(who) + 2:] for t in re.findall(r'MPG_REQUIRE\(.*?"(%s: [^"]*)"' % re.escape(who), code, flags=re.S)]


def _helper_texts(code, name_arg, seen):
    """{helper: its texts} of every `*_refusal(name_arg, ..` that `code` calls, and of those they call with their `entry` in turn"""
    out = {}
    for helper in re.findall(r'\b(\w+_refusal)\(%s' % re.escape(name_arg), code):
        if helper in seen:
            continue
        seen.add(helper)
        homes = [s for s in (open(os.path.join(CSRC, h)).read() for h in ('env_internal.h', 'gauss_head.h')) if 'inline int %s(' % helper in s]
        assert len(homes) == 1, helper
        body = homes[0][homes[0].index('inline int %s(' % helper):]
        body = body[:body.index('\n}')]
        out[helper] = _required(body, '%s')
        out.update(_helper_texts(body, 'entry', seen))
    return out


# gauss::squash_refusal's own null-pointer and row-count refusals cannot answer a rollout: it passes the head no pointer and one row
HEAD, HEAD_CANNOT_ANSWER = 'squash_refusal', ('null pointer', 'rows must be positive (got %d)')


def refusal_texts_are_unique(name, src, at_least, head_at_least=None):
    """The refusals of entry point `name` (in csrc file `src`) are told apart by their text: no two conditions share one - neither among
    the entry point's own MPG_REQUIREs, nor among those of the refusal helpers its body calls under its name (env_internal.h,
    gauss_head.h), nor between the lists.  At least `at_least` texts, gauss::squash_refusal's aside; with head_at_least the body calls
    that too, and it brings at least so many."""
    code = open(os.path.join(CSRC, src)).read()
    body = code[code.index('extern "C" int %s(' % name):]
    body = body[:body.index('hipLaunchKernelGGL')]
    shared = _helper_texts(body, '"%s"' % name, set())
    head = shared.pop(HEAD, None)
    texts = _required(body, name) + [t for h in sorted(shared) for t in shared[h]]
    assert len(texts) >= at_least, texts
    if head_at_least is not None:
        assert 'gauss::squash_refusal("%s"' % name in body
        assert head is not None and len(head) >= head_at_least, head
    if head is not None:
        texts += [t for t in head if t not in HEAD_CANNOT_ANSWER]
    assert len(set(texts)) == len(texts), texts
