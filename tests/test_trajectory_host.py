"""CPU tests of the trajectory record's plumbing (ddk_sample_trajectory, include/ddk.h): the ctypes declarations of _lib.py against the header -
the ddk_trajectory struct is the one place where a silent mismatch would make the kernels write into the wrong array - and sampling()'s argument
handling without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _header():
    return open(os.path.join(ROOT, 'include', 'ddk.h')).read()


def _ctype_of(c_decl):
    """ctypes type _lib.py must use for a C parameter / member declaration (without its name)"""
    c_decl = re.sub(r'\bconst\b', '', c_decl).strip()
    if c_decl == 'ddk_trajectory*':
        return 'POINTER(ddk_trajectory)'
    if c_decl.endswith('*'):
        return C.c_void_p
    return {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'float': C.c_float}[c_decl]


def _split_decl(d):
    """'const float* t' -> ('const float*', 't')"""
    m = re.match(r'^(.*?)([A-Za-z_][A-Za-z0-9_]*)$', d.strip())
    return m.group(1).strip(), m.group(2)


def test_trajectory_struct_matches_header():
    from disco_diffdock_amd import _lib
    m = re.search(r'typedef struct ddk_trajectory \{(.*?)\} ddk_trajectory;', _header(), re.S)
    assert m, 'include/ddk.h does not declare ddk_trajectory'
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    members = [_split_decl(d) for d in body.split(';') if d.strip()]
    assert [n for _, n in members] == ['pos', 'scores', 'perturb', 'edge_counts']
    assert [t for t, _ in members] == ['float*', 'float*', 'float*', 'int32_t*']
    assert [(n, t) for n, t in _lib.ddk_trajectory._fields_] == [(n, _ctype_of(t)) for t, n in members]
    # four pointers, no padding: the layout the library reads
    assert C.sizeof(_lib.ddk_trajectory) == 4 * C.sizeof(C.c_void_p)
    assert [getattr(_lib.ddk_trajectory, n).offset for _, n in members] == [i * C.sizeof(C.c_void_p) for i in range(4)]


def test_sample_trajectory_parameters_match_header():
    from disco_diffdock_amd import build, _lib
    from disco_diffdock_amd.runtime import TRAJECTORY_FIELDS, Trajectory
    hdr = _header()

    def params(name):
        m = re.search(r'\bint ' + name + r'\((.*?)\);', hdr, re.S)
        assert m, name
        return [_split_decl(d) for d in m.group(1).replace('\n', ' ').split(',')]
    plain, traj = params('ddk_sample'), params('ddk_sample_trajectory')
    # ddk_sample's parameters, then the record in front of the stream
    assert traj[:-2] == plain[:-1] and traj[-1] == plain[-1] == ('void*', 'stream')
    assert traj[-2] == ('const ddk_trajectory*', 'rec')
    build.build(verbose=False)
    L = _lib.lib()
    assert 'ddk_sample_trajectory' in _lib.SYMBOLS and hasattr(L, 'ddk_sample_trajectory')
    want = [_ctype_of(t) for t, _ in traj]
    got = [('POINTER(ddk_trajectory)' if a is C.POINTER(_lib.ddk_trajectory) else a) for a in L.ddk_sample_trajectory.argtypes]
    assert got == want
    assert list(L.ddk_sample.argtypes) == [_ctype_of(t) for t, _ in plain]
    # the Python container names the struct's members, in its order
    assert TRAJECTORY_FIELDS == tuple(n for n, _ in _lib.ddk_trajectory._fields_) == Trajectory._fields


def test_stale_library_is_refused_with_the_rebuild_message(monkeypatch):
    """A libddk.so that lacks a declared symbol (built from older sources) fails when it is loaded, with the message that says how to build, not with an
    AttributeError at the first call of the missing entry."""
    from disco_diffdock_amd import build, _lib
    build.build(verbose=False)
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'SYMBOLS', _lib.SYMBOLS + ['ddk_entry_of_a_newer_header'])
    with pytest.raises(RuntimeError, match=r'ddk_entry_of_a_newer_header.*python -m disco_diffdock_amd\.build'):
        _lib.lib()


def test_host_only_context_refuses_sample_trajectory():
    """the new entry has ddk_sample's refusals: a context without a device launches nothing (status + message, no crash)"""
    from disco_diffdock_amd import build, _lib
    from disco_diffdock_amd.runtime import Context
    build.build(verbose=False)
    ctx = Context(device=-1)
    ctx.finalize()
    rec = _lib.ddk_trajectory()
    rc = ctx.L.ddk_sample_trajectory(ctx.h, None, 1, 1, None, None, None, None, None, C.byref(rec), None)
    assert rc == -3 and b'host-only' in ctx.L.ddk_last_error(ctx.h)
    assert ctx.L.ddk_sample_trajectory(None, None, 1, 1, None, None, None, None, None, None, None) == -1


class _Vis:
    def add(self, *a, **k):
        raise AssertionError('no pose can exist without a GPU')


@pytest.mark.parametrize('vis', [None, [_Vis()]])
def test_sampling_on_a_cpu_device_still_raises_gpu_only(vis):
    from argparse import Namespace
    from disco_diffdock_amd.sampling import sampling
    from disco_diffdock_amd.diffusion_utils import get_t_schedule
    args = Namespace(tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.03, tor_sigma_max=3.14, no_torsion=False)
    sched = get_t_schedule(2)
    with pytest.raises(RuntimeError, match='GPU only'):
        sampling([], object(), 2, sched, sched, sched, torch.device('cpu'), lambda *a: a, args, visualization_list=vis, trajectory=[])
