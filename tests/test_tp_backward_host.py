"""CPU tests of ddk_tp_backward's host side: the closed-form restatement the kernel is written against (tests/tp_backward_ref.py) equals autograd of
the unmodified reference class (tests/golden/faster_tp_backward_l*.npz), the entry point is declared, exported and bound, and a context without a
device refuses it."""
import ctypes
import os
import re

import numpy as np
import pytest

import tp_backward_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize('l', range(5))
def test_restatement_equals_reference_autograd(golden, l):
    z = golden(f'faster_tp_backward_l{l}')
    s = ref.shape(l)
    assert z['x'].shape == (16, s['din']) and z['w'].shape == (16, s['W']) and z['grad_out'].shape == (16, s['dout'])
    assert all(z[k].dtype == np.float32 for k in ('x', 'sh', 'w', 'grad_out')) and all(z[k].dtype == np.float64 for k in ('grad_x', 'grad_sh', 'grad_w'))
    gx, gsh, gw = ref.backward(l, z['x'], z['sh'], z['w'], z['grad_out'])
    for name, got in (('grad_x', gx), ('grad_sh', gsh), ('grad_w', gw)):
        assert got.shape == z[name].shape
        assert np.abs(got - z[name]).max() < 1e-12, name
    # the adjoint identity of a trilinear map, on the restatement's own forward
    lhs = (ref.forward(l, z['x'], z['sh'], z['w']) * z['grad_out'].astype(np.float64)).sum(1)
    for got, op in ((gx, z['x']), (gsh, z['sh']), (gw, z['w'])):
        assert np.abs((got * op).sum(1) - lhs).max() < 1e-11


def test_entry_point_is_declared_exported_and_bound(built):
    from disco_diffdock_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    assert re.search(r'\bint\s+ddk_tp_backward\s*\(', hdr)
    assert 'ddk_tp_backward' in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(built), 'ddk_tp_backward')
    L = _lib.lib()
    assert len(L.ddk_tp_backward.argtypes) == 11
    assert L.ddk_tp_backward.argtypes[6] is ctypes.c_int64 and L.ddk_tp_backward.argtypes[1] is ctypes.c_int32


def test_host_only_context_refuses_backward(built):
    from disco_diffdock_amd.runtime import Context
    ctx = Context(device=-1)
    ctx.finalize()
    one = ctypes.c_void_p(16)      # never dereferenced: the refusal comes first
    rc = ctx.L.ddk_tp_backward(ctx.h, 3, one, one, one, one, 4, one, one, one, None)
    assert rc == -3 and b'host-only' in ctx.L.ddk_last_error(ctx.h)
    rc = ctx.L.ddk_tp_backward(ctx.h, 3, None, None, None, None, 4, None, None, None, None)      # all outputs null: still a refusal, not a crash
    assert rc != 0 and ctx.L.ddk_last_error(ctx.h)
    rc = ctx.L.ddk_tp_backward(ctx.h, 3, None, None, None, None, 0, None, None, None, None)
    assert rc != 0
    with pytest.raises(RuntimeError, match='at least one gradient'):
        ctx.tp_backward(3, None, None, None, None, need=(False, False, False))
    assert [ctx.tp_weight_numel(l) for l in range(5)] == [ref.shape(l)['W'] for l in range(5)]


@pytest.mark.parametrize('l', range(5))
def test_one_shape_table(built, l):
    """the package's statement of a layer's shape (runtime.tp_layer_shape), this suite's (tp_backward_ref.shape) and the kernels' (csrc/k_tp_shape.h,
    read through the workspace size of one slice of one group: W rows of 72 + 1 floats) are the same table"""
    from disco_diffdock_amd import _lib
    from disco_diffdock_amd.runtime import tp_layer_shape
    got, want = tp_layer_shape(l), ref.shape(l)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    assert _lib.lib().ddk_rtp_backward_workspace(l, 0, 1) == want['W'] * 73 * 4
