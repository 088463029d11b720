"""CPU tests of the radial tensor product's host side: the closed form the kernels are written against (tests/radial_tp_ref.py) equals autograd of the
unmodified reference classes (tests/golden/radial_tp_l0.npz), the three entry points are declared, exported and bound, the workspace is a bounded function
of its arguments, and a context without a device refuses the launches."""
import ctypes
import os
import re

import numpy as np
import pytest

import radial_tp_ref as ref
import tp_backward_ref as tpr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
ENTRIES = ('ddk_rtp_forward', 'ddk_rtp_backward', 'ddk_rtp_backward_workspace')


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


def test_closed_form_equals_reference_autograd(golden):
    z = golden('radial_tp_l0')
    s = tpr.shape(0)
    offs = [int(o) for o in z['offsets']]
    assert offs == [0, 11, 24] and z['x'].shape == (24, s['din']) and z['h'].shape == (24, 72) and z['w2'].shape == (2, s['W'], 72) and z['b2'].shape == (2, s['W'])
    assert all(z[k].dtype == np.float32 for k in ('x', 'sh', 'h', 'w2', 'b2', 'grad_out'))
    assert all(z[k].dtype == np.float64 for k in ('out', 'grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2'))
    ops = (z['x'], z['sh'], z['h'], offs, z['w2'], z['b2'])
    out = ref.forward(0, *ops)
    assert out.shape == z['out'].shape and np.abs(out - z['out']).max() < 1e-12
    got = ref.backward(0, *ops, z['grad_out'])
    for name, a in zip(('grad_x', 'grad_sh', 'grad_h', 'grad_w2', 'grad_b2'), got):
        assert a.shape == z[name].shape, name
        assert np.abs(a - z[name]).max() < 1e-12, name
        assert np.abs(z[name]).max() > 0.1, name


def test_golden_is_no_larger_than_the_largest_golden():
    d = os.path.join(ROOT, 'tests', 'golden')
    sizes = {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith('.npz')}
    assert sizes['radial_tp_l0.npz'] <= max(v for f, v in sizes.items() if f != 'radial_tp_l0.npz')


def test_entry_points_are_declared_exported_and_bound(built):
    from disco_diffdock_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    assert re.search(r'\bint\s+ddk_rtp_forward\s*\(', hdr) and re.search(r'\bint\s+ddk_rtp_backward\s*\(', hdr)
    assert re.search(r'\bint64_t\s+ddk_rtp_backward_workspace\s*\(', hdr)
    cdll = ctypes.CDLL(built)
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and hasattr(cdll, name), name
    L = _lib.lib()
    assert len(L.ddk_rtp_forward.argtypes) == 12 and len(L.ddk_rtp_backward.argtypes) == 18 and len(L.ddk_rtp_backward_workspace.argtypes) == 3
    assert L.ddk_rtp_forward.argtypes[9] is ctypes.c_int64 and L.ddk_rtp_backward.argtypes[10] is ctypes.c_int64
    assert L.ddk_rtp_backward_workspace.restype is ctypes.c_int64
    from disco_diffdock_amd import tensor_layers
    from disco_diffdock_amd.runtime import Context
    assert callable(tensor_layers.fused_radial_tp) and callable(Context.rtp_forward) and callable(Context.rtp_backward)


def test_workspace_is_bounded_and_refuses_bad_arguments(built):
    from disco_diffdock_amd import _lib
    ws = _lib.lib().ddk_rtp_backward_workspace
    image = lambda l: tpr.shape(l)['W'] * 73 * 4
    for l in range(5):
        assert ws(l, 0, 1) == image(l) and ws(l, 0, 4) == 4 * image(l)
        prev = 0
        for E in (1, 511, 512, 513, 5000, 50000, 122880, 122881, 800000, 10 ** 7, 2 ** 31 - 1):
            b = ws(l, E, 4)
            assert 0 < b <= 160 * 10 ** 6 and b % image(l) == 0, (l, E, b)      # whole partial images, at most 160 MB whatever E is
            assert b >= prev or E > 122880      # (past 122 880 edges the slices grow instead of their number)
            prev = b
    assert ws(3, 50000, 4) < 4 * 50000 * tpr.shape(3)['W'] // 4      # far below one [E, W] tensor at the size of the memory test
    assert ws(3, 10 ** 7, 4) == ws(3, 10 ** 7, 4)
    for bad in ((-1, 10, 4), (5, 10, 4), (3, -1, 4), (3, 2 ** 31, 4), (3, 10, 0), (3, 10, 5)):
        assert ws(*bad) == -1, bad


def test_host_only_context_refuses_the_launches(built):
    from disco_diffdock_amd.runtime import Context
    ctx = Context(device=-1)
    ctx.finalize()
    one = ctypes.c_void_p(16)      # never dereferenced: the refusal comes first
    offs = (ctypes.c_int64 * 2)(0, 4)
    rc = ctx.L.ddk_rtp_forward(ctx.h, 3, one, one, one, offs, 1, one, one, 4, one, None)
    assert rc == -3 and b'host-only' in ctx.L.ddk_last_error(ctx.h)
    rc = ctx.L.ddk_rtp_backward(ctx.h, 3, one, one, one, offs, 1, one, one, one, 4, one, one, one, one, one, one, None)
    assert rc == -3 and b'host-only' in ctx.L.ddk_last_error(ctx.h)
    with pytest.raises(RuntimeError, match='at least one gradient'):
        ctx.rtp_backward(3, None, None, None, [0, 0], None, None, None, need=(False,) * 5)
