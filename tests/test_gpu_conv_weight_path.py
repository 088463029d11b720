"""How the default conv kernel (ddk_config.conv_kernel = 0, k_conv_x2.hip) gets its weights: the two-limb tile records in the LDS ring (9 360 B, the second
16-B chunk moved by threads 0..72 only) and, in the node-term split instantiations, GEMM1's fragments resident in LDS and reloaded when a workgroup's next
unit belongs to another weight group.

* Few workgroups (ddk_debug_set_conv_workgroups): at one workgroup per CU a small case gives every workgroup at most one unit, so the reload and the ring's
  hand-over between units of different groups only happen with a handful of workgroups.  Deterministic mode must give the same BITS at 1, 3 and the default
  number of workgroups (sample-aligned units: the result does not depend on which workgroup ran a unit); the default mode must agree with the CPU oracle and
  with the three-limb form (conv_kernel = 3: its own records, GEMM1 fragments from global memory) at the suite's 1e-4 bar; a latent-conditioned context runs
  the patch group's mapped weight group through the same reload.
* Every layer shape through ddk_conv_forward (the instantiation without the node-term split: new W2 records, GEMM1 fragments from global memory) on groups
  that are empty, partial and no multiple of the 256-edge unit.

Every Context names its conv_kernel and deterministic, so the file means the same under DDK_CONV_KERNEL / DDK_DETERMINISTIC."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import score_model_ref as smr
from oracle import sampler_ref as spr
from helpers import batch_of, chan_err, elem_err, rel_err

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CFG = smr.ScoreModelConfig(latent_vocab=64)
B = 3
WORKGROUPS = (None, 3, 1)      # None: the default (one per CU), first, because the hook has no "back to default"


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _case():
    from disco_diffdock_amd import synthetic
    c = synthetic.make_complex(31, n_res=40, n_lig=10)
    rng = np.random.default_rng(3)
    pos = np.stack([c['lig_pos'] + rng.normal(0, 4.0, size=(1, 3)) + rng.normal(0, 0.3, size=c['lig_pos'].shape) for _ in range(B)]).astype(np.float32)
    return c, pos, smr.random_state_dict(CFG, seed=5)


@functools.lru_cache(maxsize=None)
def _oracle(t):
    """the CPU oracle's scores and ligand rows of the small case, computed once per diffusion time"""
    c, pos, P = _case()
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', 'disco_diffdock_amd', 'data'))
    so3, torus = np.load(os.path.join(root, 'so3_exp_score_norms.npy')), np.load(os.path.join(root, 'torus_score_norm_seed0.npy'))
    b = batch_of(c, B, pos)
    spr.set_time(b, t, t, t, B)
    tr, rot, tor, inter = smr.score_model_forward(P, CFG, b, so3, torus, return_intermediates=True)
    return tr, rot, tor, inter['lig_node_attr']


def _set_workgroups(ctx, n):
    if n is not None:
        ctx._check(ctx.L.ddk_debug_set_conv_workgroups(ctx.h, n), 'ddk_debug_set_conv_workgroups')


def _forward(cx, pos, t, dev):
    tr, rot, tor = cx.score_forward(pos, t, t, t)
    return tr.cpu(), rot.cpu(), tor.cpu().reshape(-1), cx.lig_node_features(B, dev).cpu()


NAMES = ('tr', 'rot', 'tor', 'lig_node_attr')


@pytest.mark.parametrize('t', [1.0, 0.05])
def test_few_workgroups_meet_several_weight_groups(dev, t):
    """score_forward of a 3-sample, 40-residue complex at 1, 3 and the default number of conv workgroups.  Deterministic mode: torch.equal between the three.
    Default mode: every one within 1e-4 of the CPU oracle (scores: relative; ligand rows: per channel) and of a conv_kernel = 3 context (1e-4 relative: the two
    forms differ by their limb arithmetic and the order of the atomics only, both far below the bar each is held to against the oracle)."""
    from disco_diffdock_amd.runtime import Context, Complex
    c, pos_np, P = _case()
    pos = T(pos_np).to(dev)
    ref = _oracle(t)

    det = Context(device=0, deterministic=1, conv_kernel=0)
    det.load_state_dict(P)
    cxd = Complex(det, c, B)
    bits = []
    for n in WORKGROUPS:
        _set_workgroups(det, n)
        bits.append(_forward(cxd, pos, t, dev))
    for n, got in zip(WORKGROUPS[1:], bits[1:]):
        for name, a, b in zip(NAMES, got, bits[0]):
            assert torch.equal(a, b), (t, n, name, float((a - b).abs().max()))
    assert all(bool(torch.isfinite(x).all()) for x in bits[0]) and float(bits[0][3].abs().max()) > 0
    cxd.close()
    det.close()

    six = Context(device=0, deterministic=0, conv_kernel=3)
    six.load_state_dict(P)
    cx6 = Complex(six, c, B)
    want6 = _forward(cx6, pos, t, dev)
    ctx = Context(device=0, deterministic=0, conv_kernel=0)
    ctx.load_state_dict(P)
    cx = Complex(ctx, c, B)
    for n in WORKGROUPS:
        _set_workgroups(ctx, n)
        got = _forward(cx, pos, t, dev)
        errs = {name: (rel_err(got[k], ref[k].reshape(got[k].shape)) if k < 3 else chan_err(got[k], ref[k])) for k, name in enumerate(NAMES)}
        errs6 = {name: rel_err(got[k], want6[k]) for k, name in enumerate(NAMES)}
        print(f'conv workgroups {n} t={t}: vs oracle {errs}, vs conv_kernel 3 {errs6}')
        assert all(e < 1e-4 for e in errs.values()), (t, n, errs)
        assert all(e < 1e-4 for e in errs6.values()), (t, n, errs6)
    for x in (cx, cx6):
        x.close()
    for x in (ctx, six):
        x.close()


def test_few_workgroups_disco_patch_group_reloads(dev):
    """Latent-conditioned model, two one-hot residue picks per sample: layer 0's patch group runs with a MAPPED weight group (ConvLaunch::wmap), which a workgroup
    meets behind units of other groups when there are few of them.  The shared pass + patches must equal the full evaluation (ddk_debug_set_layer0_dedup(0))
    under the bound of test_gpu_round2.py::test_disco_layer0_patches_equal_full, 1e-5, at 1, 3 and the default number of workgroups."""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    cfg = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    c = synthetic.make_complex(32, n_res=40, n_lig=10)
    ctx = Context(device=0, latent_dim=2, latent_vocab=1, latent_droprate=0.1, deterministic=0, conv_kernel=0)
    ctx.load_state_dict(smr.random_state_dict(cfg, seed=9))
    rng = np.random.default_rng(6)
    pos = T(np.stack([c['lig_pos'] + rng.normal(0, 4.0, size=(1, 3)) for _ in range(B)]).astype(np.float32)).to(dev)
    cx = Complex(ctx, c, B)
    n_l, n_r = cx.n_lig, cx.n_rec
    ll, lr = torch.zeros(B * n_l, 2), torch.zeros(B * n_r, 2)
    for s in range(B):
        for d in range(2):
            lr[s * n_r + rng.integers(n_r), d] = 1
    ll, lr = ll.to(dev), lr.to(dev)
    for n in WORKGROUPS:
        _set_workgroups(ctx, n)
        for t in (1.0, 0.05):
            res = {}
            for on in (True, False):
                ctx.debug_set_layer0_dedup(on)
                cx.set_latents(ll, lr, 0.0)
                res[on] = _forward(cx, pos, t, dev)
                if on:
                    cnt, mask = cx.debug_read_patch(B)
                    assert cnt[B] > 0 and mask[1:].any() and not mask[0].any()      # the patch group is what ran
            ctx.debug_set_layer0_dedup(True)
            errs = {name: rel_err(res[True][k], res[False][k]) for k, name in enumerate(NAMES)}
            print(f'DisCo patches vs full, conv workgroups {n} t={t}: {errs}')
            assert all(e < 1e-5 for e in errs.values()), (n, t, errs)
    cx.close()
    ctx.close()


@pytest.mark.parametrize('l', range(5))
def test_conv_forward_partial_and_empty_groups(dev, l):
    """ddk_conv_forward of every layer shape on 703 edges in four groups of 130 / 0 / 301 / 272 (one empty, one a unit and a bit, none a multiple of 256: partial
    units, waves past a group's end, the column split of the last blocks) against the fp64 oracle, under the two conditions of
    test_gpu_round6.py::test_two_limb_kernel_is_fp32_grade: under 1e-5 relative, and within 1.5 x the error of the fp32-MFMA chains (conv_kernel = 1) measured here."""
    from disco_diffdock_amd.runtime import Context
    from test_gpu_ops import _random_case, CFG as OCFG
    N, splits = 60, [0, 130, 130, 431, 703]
    i_irr, o_irr = OCFG.conv_irreps(l)
    Pl = smr.random_conv_layer_params(OCFG, l, 521 + l, True)
    node, ei, ea, sh = _random_case(l, N, splits, 19 + l, True)
    P = {'L.' + k: v.double() for k, v in Pl.items()}
    ref = smr.tp_conv_layer(P, 'L', node.double(), ei, [ea.double()[splits[i]:splits[i + 1]] for i in range(4)], sh.double(),
                            i_irr, '1x0e+1x1o', o_irr, residual=True, batch_norm=True, faster=True, edge_groups=4)
    args = (l, node.to(dev), ei[0].to(dev), ei[1].to(dev), splits, ea.to(dev), sh.to(dev), smr.irreps_dim(o_irr))
    err = {}
    for kernel in (0, 1):
        ctx = Context(device=0, conv_kernel=kernel, deterministic=0)
        assert int(ctx.cfg.conv_kernel) == kernel
        ctx.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in Pl.items()})
        out = ctx.conv_forward(*args).cpu()
        err[kernel] = (rel_err(out, ref), elem_err(out, ref))
        ctx.close()
    print(f'conv layer {l}, 703 edges vs fp64: two limbs (default) {err[0]}, fp32 MFMA chains {err[1]}')
    assert err[0][0] < 1e-5 and err[0][0] <= 1.5 * err[1][0] and err[0][1] <= 1.5 * err[1][1], err
