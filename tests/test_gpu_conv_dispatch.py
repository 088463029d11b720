"""The conv dispatch (csrc/conv_launch.hip: conv_select) on the paths no other test reaches: the TRACE instantiation of the f16-limb kernels,
and the contexts on which a trace pointer is ignored - the fp32 kernel (conv_kernel = 1) and a deterministic launch (det comes before trace).

One reference-produced golden (complex_diffdockS_score_model, score at t = 0.55: a ligand of a few dozen atoms), the weights of
random_state_dict(CFG, seed=7), and the bar test_core_parity_in_every_mode applies to it: elem_err < 1e-4 on tr / rot / tor.  Every context
names its conv_kernel and deterministic (keyword arguments win over DDK_CONV_KERNEL / DDK_DETERMINISTIC), so the file means the same under
the environment switches."""
import ctypes as C

import pytest
import torch

from oracle import score_model_ref as smr
from helpers import complex_from_npz, elem_err

pytestmark = pytest.mark.gpu
CFG = smr.ScoreModelConfig(latent_vocab=64)
TAG, TIME, LAYER = 'diffdockS_score_model', 0.55, 1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def case(dev, golden):
    """(golden scores, device batch) shared by every test of the file"""
    from test_gpu_model import _dev_batch
    z = golden(f'score_{TAG}_t{TIME}')
    c = complex_from_npz(golden(f'complex_{TAG}'))
    return z, _dev_batch(c, int(z['B']), z['pos'], dev, TIME)


def _score_model(dev, conv_kernel, deterministic):
    from functools import partial
    from test_gpu_model import ARGS_S
    from disco_diffdock_amd.model_utils import get_model
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    from disco_diffdock_amd.runtime import Context
    sm = get_model(ARGS_S, dev, partial(t_to_sigma, args=ARGS_S), no_parallel=True).score_model
    sm.ctx.close()
    sm.cfg.update(conv_kernel=conv_kernel, deterministic=deterministic)
    sm.ctx = Context(device=0, **sm.cfg)
    assert (int(sm.ctx.cfg.conv_kernel), int(sm.ctx.cfg.deterministic)) == (conv_kernel, deterministic)
    sm.load_state_dict(smr.random_state_dict(CFG, seed=7), strict=True)
    return sm


def _forward(sm, case):
    """one forward; the scores meet the bar of the goldens; returns them (host copies)"""
    z, b = case
    out = [a.cpu().clone() for a in sm(b)]
    for name, a in zip(('tr', 'rot', 'tor'), out):
        assert elem_err(a, z[name]) < 1e-4, name
    return out


def _trace(sm, layer, buf):
    sm.ctx._check(sm.ctx.L.ddk_debug_conv_trace(sm.ctx.h, layer, C.c_void_p(buf.data_ptr()) if buf is not None else None), 'ddk_debug_conv_trace')


def _buffer(dev):
    return torch.zeros((8, 1024, 8), dtype=torch.int32, device=dev)      # [wave][tile][stamp] uint32 (ddk_debug.h)


@pytest.mark.parametrize('conv_kernel', [0, 3], ids=['x2', 'x3'])
def test_trace_instantiation_runs_and_stamps(dev, case, conv_kernel):
    """f16-limb kernels, atomics: the traced layer runs conv_x2 / conv_x3_kernel<1, 1, 0, TRACE> - same scores, workgroup 0 writes its stamps;
    with the hook off the plain kernel runs again and nothing is written."""
    sm = _score_model(dev, conv_kernel, 0)
    buf = _buffer(dev)
    _trace(sm, LAYER, buf)
    _forward(sm, case)
    assert bool((buf[0, 0] != 0).any()), 'wave 0 wrote no stamp into its first record'
    _trace(sm, -1, None)
    fresh = _buffer(dev)      # (a stale pointer would be `buf`; a kernel that still traced would have nowhere else to write)
    before = buf.clone()
    _forward(sm, case)
    assert not bool(fresh.any()) and torch.equal(buf, before)


@pytest.mark.parametrize('conv_kernel,deterministic', [(1, 0), (0, 1)], ids=['fp32-atomics', 'x2-deterministic'])
def test_trace_pointer_is_ignored(dev, case, conv_kernel, deterministic):
    """The fp32 family has no TRACE kernel and det comes before trace: the forward succeeds, meets the bar and leaves the buffer alone; the
    deterministic forward gives the bits of an untraced one."""
    sm = _score_model(dev, conv_kernel, deterministic)
    plain = _forward(sm, case)
    buf = _buffer(dev)
    _trace(sm, LAYER, buf)
    traced = _forward(sm, case)
    _trace(sm, -1, None)
    assert not bool(buf.any())
    if deterministic:
        for a, b in zip(plain, traced):
            assert torch.equal(a, b)
