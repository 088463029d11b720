"""GPU tests of the device-side trajectory record (ddk_sample_trajectory, include/ddk.h; Complex.sample(record=...); sampling(visualization_list=...,
trajectory=...)): the sampler's own launches store the poses before every step, the scores and perturbations every update consumed and the edge counts
of every step's graph.

* the record of ONE 20-step call against oracle.sampler_ref's trace (pocket-bound setting of test_pocket_bound_trajectory_vs_oracle), plain and guided steps;
* recording changes no pose bit; `perturb` is score_coeff * score + noise_coeff * z to fp32 rounding; `edge_counts` equals ddk_last_graph_stats step by step;
* argument handling, rigid and no_torsion records, and the reference's visualization_list call pattern."""
import ctypes as C
from argparse import Namespace
from functools import partial

import numpy as np
import pytest
import torch

from oracle import score_model_ref as smr
from oracle import sampler_ref as spr
from helpers import rel_err, to_graph

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CFG = smr.ScoreModelConfig(latent_vocab=64)
ARGS = Namespace(tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.03, tor_sigma_max=3.14, no_torsion=False)
POSE_BAR, STEP_BAR = 1e-3, 1e-4      # the bars test_pocket_bound_trajectory_vs_oracle carries: poses (rel_err, receptor scale), per-step vectors (rel_err)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def _coefficients(steps):
    from test_gpu_model import README_S
    from disco_diffdock_amd.sampling import step_coefficients
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    sched = get_t_schedule(steps)
    return (sched,) + step_coefficients(steps, sched, sched, sched, partial(t_to_sigma, args=ARGS), ARGS, False, False, True, README_S['temp_sampling'],
                                        README_S['temp_psi'], README_S['temp_sigma_data'])


def _pocket_poses(c, B, seed):
    """start poses inside the pocket: rotation about the centroid + N(0, 1 A) (bench.py's pocket-bound bracket)"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    lp = c['lig_pos'].astype(np.float64)
    ctr = lp.mean(0, keepdims=True)
    return np.stack([(lp - ctr) @ Rotation.random(random_state=rng).as_matrix().T + ctr + rng.normal(0, 1.0, size=(1, 3)) for _ in range(B)]).astype(np.float32)


def _oracle_trace(c, P, cfg, tables, pos0, z, sub, steps, sched, per_graph=None, **kw):
    """oracle.sampler_ref.sampling(..., trace=[]) on the samples `sub` with the device's noise -> (trace, final poses [len(sub) * n, 3])"""
    from test_gpu_model import README_S
    dl = []
    for i in sub:
        g = to_graph(c)
        g['ligand'].pos = T(pos0[i])
        if per_graph is not None:
            per_graph(g, i)
        dl.append(g)
    zs = z[:, sub]
    nf = lambda b, t, name, shape: {'tr': zs[t, :, 0:3], 'rot': zs[t, :, 3:6], 'tor': zs[t, :, 6:].reshape(-1)}[name]
    trace = []
    ref, _ = spr.sampling(dl, P, cfg, tables[0], tables[1], steps, sched, sched, sched, noise_fn=nf, batch_size=len(dl), no_final_step_noise=True, trace=trace,
                          **README_S, **kw)
    return trace, torch.cat([g['ligand'].pos for g in ref])


def _compare_with_trace(rec, trace, final, sub, steps):
    """-> maxima over the steps of rel_err(record, oracle trace) for the poses (incl. the final row), the scores and the perturbations"""
    pos, scores, perturb = rec.pos.cpu()[:, sub], rec.scores.cpu()[:, sub], rec.perturb.cpu()[:, sub]
    e_pos = [rel_err(pos[k].reshape(-1, 3), trace[k]['pos']) for k in range(steps)] + [rel_err(pos[steps].reshape(-1, 3), final)]
    e_sc, e_pt = [], []
    for k in range(steps):
        for arr, out, names in ((scores, e_sc, ('tr_score', 'rot_score', 'tor_score')), (perturb, e_pt, ('tr_perturb', 'rot_perturb', 'tor_perturb'))):
            parts = (arr[k][:, 0:3], arr[k][:, 3:6], arr[k][:, 6:].reshape(-1))
            out.append(max(rel_err(a, trace[k][nm]) for a, nm in zip(parts, names) if trace[k][nm] is not None and trace[k][nm].numel()))
    return e_pos, e_sc, e_pt


def test_recorded_trajectory_vs_oracle_inside_one_call(dev, tables):
    """The setting of test_pocket_bound_trajectory_vs_oracle (300 residues, B = 40, README low-temperature coefficients, supplied noise scaled by 0.2,
    no_final_step_noise), but the 20 steps run in ONE Complex.sample(record=True) call - the product path, heads' post fused into the update - and every
    per-step quantity is read from the record: pos[k] vs the oracle trace's `pos`, scores[k] vs tr / rot / tor_score, perturb[k] vs *_perturb, pos[steps] vs
    the oracle's final poses, on four of the samples.  Bars as in that test: poses 1e-3, per-step vectors 1e-4 of each vector's largest element."""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    c = synthetic.make_complex(0, n_res=300)
    P = smr.random_state_dict(CFG, seed=21)
    ctx = Context(device=0)
    ctx.load_state_dict(P)
    B, steps = 40, 20
    cx = Complex(ctx, c, B)
    sched, t_arr, sc, nc = _coefficients(steps)
    pos0 = _pocket_poses(c, B, 1000)
    z = 0.2 * torch.randn(steps, B, 6 + cx.R, generator=torch.Generator().manual_seed(19))
    sub = [0, 13, 26, 39]
    pos = T(pos0.copy()).to(dev)
    rec = cx.sample(pos, t_arr, sc, nc, z.to(dev), record=True)
    torch.cuda.synchronize()
    assert tuple(rec.pos.shape) == (steps + 1, B, cx.n_lig, 3) and tuple(rec.scores.shape) == tuple(rec.perturb.shape) == (steps, B, 6 + cx.R)
    assert tuple(rec.edge_counts.shape) == (steps, 4) and rec.edge_counts.dtype == torch.int32
    assert torch.equal(rec.pos[0].cpu(), T(pos0)) and torch.equal(rec.pos[steps], pos)
    cross = rec.edge_counts.cpu()[:, 1].double() / B
    assert float(cross.min()) >= 2500, cross          # the premise of the setting: every step is pocket bound
    trace, final = _oracle_trace(c, P, CFG, tables, pos0, z, sub, steps, sched)
    e_pos, e_sc, e_pt = _compare_with_trace(rec, trace, final, sub, steps)
    print(f'recorded 20-step trajectory, B = 40 (oracle on samples {sub}): poses max {max(e_pos):.2e} (final {e_pos[-1]:.2e}), scores max {max(e_sc):.2e}, '
          f'perturbations max {max(e_pt):.2e}; cross edges per sample {float(cross.min()):.0f} .. {float(cross.max()):.0f}')
    assert max(e_pos) < POSE_BAR and max(e_sc) < STEP_BAR and max(e_pt) < STEP_BAR, (e_pos, e_sc, e_pt)


def test_recorded_guided_steps_vs_oracle(dev, tables):
    """A latent-conditioned context (latent_dim = 2, one-hot latents bound by hand) with classifier-free guidance on a window that covers steps 2 and 3 of 5
    (t = 0.6, 0.4): one recorded call runs the fused <heads' post + update> kernel on the plain steps and the update behind cfg_combine on the guided ones.
    The recorded scores are the COMBINED ones (utils/sampling.py:131-133) and agree with the oracle trace run with the same weight and window; same bars."""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    cfg = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    P = smr.random_state_dict(cfg, seed=13)
    c = synthetic.make_complex(31, n_res=40, n_lig=22)
    ctx = Context(device=0, latent_dim=2, latent_vocab=1, latent_droprate=0.1)
    ctx.load_state_dict(P)
    B, steps = 3, 5
    guide = dict(classifier_free_guidance_weight=0.7, cfg_start=0.7, cfg_end=0.3)
    cx = Complex(ctx, c, B)
    n_l, n_r = cx.n_lig, cx.n_rec
    rng = np.random.default_rng(2)
    ll, lr = torch.zeros(B * n_l, 2), torch.zeros(B * n_r, 2)
    for s in range(B):
        lr[s * n_r + rng.integers(n_r), 0] = 1
        (ll if s == 1 else lr)[s * (n_l if s == 1 else n_r) + rng.integers(n_l if s == 1 else n_r), 1] = 1
    cx.set_latents(ll.to(dev), lr.to(dev), 0.0)
    cx.set_guidance(guide['classifier_free_guidance_weight'], guide['cfg_start'], guide['cfg_end'])
    sched, t_arr, sc, nc = _coefficients(steps)
    guided = [bool(guide['cfg_end'] <= t <= guide['cfg_start']) for t in sched]
    assert guided == [False, False, True, True, False]
    pos0 = np.stack([c['lig_pos'] + rng.normal(0, 2.0, size=(1, 3)) for _ in range(B)]).astype(np.float32)
    z = 0.2 * torch.randn(steps, B, 6 + cx.R, generator=torch.Generator().manual_seed(5))
    pos = T(pos0.copy()).to(dev)
    rec = cx.sample(pos, t_arr, sc, nc, z.to(dev), record=True)
    torch.cuda.synchronize()
    assert torch.equal(rec.pos[0].cpu(), T(pos0)) and torch.equal(rec.pos[steps], pos)
    assert int(rec.edge_counts.cpu()[:, 1].min()) > 0          # every step saw cross edges

    def bind(g, i):
        g['ligand'].latent_h, g['receptor'].latent_h = ll[i * n_l:(i + 1) * n_l], lr[i * n_r:(i + 1) * n_r]
        g['ligand'].unconditional, g['receptor'].unconditional = torch.zeros(n_l, 1), torch.zeros(n_r, 1)
    sub = list(range(B))
    trace, final = _oracle_trace(c, P, cfg, tables, pos0, z, sub, steps, sched, per_graph=bind, **guide)
    e_pos, e_sc, e_pt = _compare_with_trace(rec, trace, final, sub, steps)
    print(f'recorded guided trajectory (guided steps {[k for k, g in enumerate(guided) if g]}): poses max {max(e_pos):.2e}, scores per step '
          f'{[f"{e:.1e}" for e in e_sc]}, perturbations max {max(e_pt):.2e}')
    assert max(e_pos) < POSE_BAR and max(e_sc) < STEP_BAR and max(e_pt) < STEP_BAR, (e_pos, e_sc, e_pt)


def _det_setup(dev, B=6, steps=20, n_res=120, **ctx_kw):
    """deterministic context (bit-identical run to run) + a 20-step pocket-bound workload on a 120-residue complex"""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    c = synthetic.make_complex(3, n_res=n_res)
    ctx = Context(device=0, deterministic=1, **ctx_kw)
    ctx.load_state_dict(smr.random_state_dict(CFG, seed=9))
    cx = Complex(ctx, c, B)
    _, t_arr, sc, nc = _coefficients(steps)
    pos0 = T(_pocket_poses(c, B, 77)).to(dev)
    z = (0.3 * torch.randn(steps, B, 6 + cx.R, generator=torch.Generator().manual_seed(3))).to(dev)
    return cx, t_arr, sc, nc, pos0, z


def _raw_sample_trajectory(cx, pos, t_arr, sc, nc, z, rec):
    """ddk_sample_trajectory with a caller-built ddk_trajectory (or None = a NULL rec)"""
    from disco_diffdock_amd.runtime import _stream
    ctx = cx.ctx
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    t_arr, sc, nc = [np.ascontiguousarray(a, np.float32) for a in (t_arr, sc, nc)]
    ctx._check(ctx.L.ddk_sample_trajectory(ctx.h, cx.h, pos.shape[0], t_arr.shape[0], p(t_arr), p(sc), p(nc), C.c_void_p(z.data_ptr()), C.c_void_p(pos.data_ptr()),
                                           None if rec is None else C.byref(rec), _stream()), 'ddk_sample_trajectory')


def test_recording_changes_no_pose_bit(dev):
    """deterministic = 1: the final poses of ddk_sample, of ddk_sample_trajectory with all four arrays, with every single array, with an all-NULL struct and with
    rec = NULL are bit-identical; pos[0] is the input and pos[steps] the returned poses, bit for bit; the single-array records equal the full one's."""
    from disco_diffdock_amd import _lib
    from disco_diffdock_amd.runtime import TRAJECTORY_FIELDS
    steps = 20
    cx, t_arr, sc, nc, pos0, z = _det_setup(dev, steps=steps)
    plain = cx.sample(pos0.clone(), t_arr, sc, nc, z)
    p_all = pos0.clone()
    full = cx.sample(p_all, t_arr, sc, nc, z, record=True)
    assert torch.equal(p_all, plain)
    assert torch.equal(full.pos[0], pos0) and torch.equal(full.pos[steps], plain)
    assert not torch.equal(full.pos[1], full.pos[0]) and not torch.equal(full.pos[steps], full.pos[steps - 1])
    for name in TRAJECTORY_FIELDS:
        p1 = pos0.clone()
        one = cx.sample(p1, t_arr, sc, nc, z, record=(name,))
        assert torch.equal(p1, plain), name
        assert [k for k in TRAJECTORY_FIELDS if getattr(one, k) is not None] == [name]
        assert torch.equal(getattr(one, name), getattr(full, name)), name
    for rec in (None, _lib.ddk_trajectory()):
        p0 = pos0.clone()
        _raw_sample_trajectory(cx, p0, t_arr, sc, nc, z, rec)
        assert torch.equal(p0, plain)
    sub = cx.sample(pos0.clone(), t_arr, sc, nc, z, record=('pos', 'edge_counts'))
    assert sub.scores is None and sub.perturb is None and torch.equal(sub.pos, full.pos) and torch.equal(sub.edge_counts, full.edge_counts)
    with pytest.raises(ValueError, match='record'):
        cx.sample(pos0.clone(), t_arr, sc, nc, z, record=('poses',))


def test_perturb_is_score_coeff_score_plus_noise_coeff_z(dev):
    """perturb[k] against sc[k] * scores[k] + nc[k] * z[k] formed on the host in fp32 from the RECORDED scores: elementwise
    |delta| <= 2 * 2^-23 * (|sc * s| + |nc * z|) - one rounding of each product and of the sum on either side, with or without FMA contraction.
    The last step (no_final_step_noise: nc = 0) has perturb = sc * score."""
    steps = 20
    cx, t_arr, sc, nc, pos0, z = _det_setup(dev, steps=steps)
    rec = cx.sample(pos0.clone(), t_arr, sc, nc, z, record=('scores', 'perturb'))
    s, pt, zz = rec.scores.cpu(), rec.perturb.cpu(), z.cpu()
    col = torch.tensor([0, 0, 0, 1, 1, 1] + [2] * cx.R)
    a = T(np.ascontiguousarray(sc, np.float32))[:, col][:, None, :] * s          # fp32 products [steps, B, 6 + R]
    b = T(np.ascontiguousarray(nc, np.float32))[:, col][:, None, :] * zz
    host = a + b
    bound = 2.0 * 2.0 ** -23 * (a.double().abs() + b.double().abs())
    delta = (pt.double() - host.double()).abs()
    worst = float((delta / bound.clamp_min(1e-300)).max())
    print(f'perturb vs host fp32 sc * s + nc * z: worst |delta| / bound = {worst:.3f} (bar 1), R = {cx.R}')
    assert cx.R > 0 and float(s[:, :, 6:].abs().min()) > 0          # the torsion columns are live
    assert bool((delta <= bound).all()), worst
    assert not nc[steps - 1].any() and torch.equal(pt[steps - 1], a[steps - 1])


def test_edge_counts_equal_graph_stats_step_by_step(dev):
    """The recorded 20-step call against the same trajectory stepped one step per call from the host with graph_stats() read after each step (deterministic
    context): integer equality of E_ll, E_lr, E_rr, E_rl at every step, and the poses of the two runs bit-identical (one step per call is the same launches)."""
    steps = 20
    cx, t_arr, sc, nc, pos0, z = _det_setup(dev, steps=steps)
    p_rec = pos0.clone()
    rec = cx.sample(p_rec, t_arr, sc, nc, z, record=('edge_counts', 'pos'))
    got = rec.edge_counts.cpu().tolist()
    p_step, want = pos0.clone(), []
    for k in range(steps):
        assert torch.equal(rec.pos[k], p_step), k
        cx.sample(p_step, t_arr[k:k + 1], sc[k:k + 1], nc[k:k + 1], z[k:k + 1])
        st = cx.graph_stats()
        want.append([st['E_ll'], st['E_lr'], st['E_rr'], st['E_rl']])
    print(f'edge counts per step (E_ll, E_lr, E_rr, E_rl): first {got[0]}, last {got[-1]}')
    assert got == want
    assert torch.equal(p_rec, p_step)
    assert len({tuple(g) for g in got}) > 1 and all(g[1] == g[3] and g[1] > 0 for g in got)          # the counts move, lr and rl mirror each other


def test_sample_trajectory_refuses_bad_arguments(dev):
    """steps < 1, B above the complex's max_batch and a confidence_mode context are refused with a message, like ddk_sample"""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Complex
    from test_gpu_round4 import _cg_conf_model
    cx, t_arr, sc, nc, pos0, z = _det_setup(dev, B=2, steps=3, n_res=40)
    with pytest.raises(RuntimeError, match='ddk_sample_trajectory'):
        cx.sample(pos0.clone(), t_arr[:0], sc[:0], nc[:0], z[:0], record=True)
    big = torch.cat([pos0, pos0[:1]])
    with pytest.raises(RuntimeError, match='max_batch'):
        cx.sample(big, t_arr, sc, nc, torch.cat([z, z[:, :1]], dim=1), record=True)
    cm, _ = _cg_conf_model(dev, 3)
    cxc = Complex(cm.score_model.ctx, synthetic.make_complex(3, n_res=40), 2)
    pc = T(_pocket_poses(synthetic.make_complex(3, n_res=40), 2, 1)).to(dev)
    with pytest.raises(RuntimeError, match='confidence_mode'):
        cxc.sample(pc, t_arr, sc, nc, None, record=True)
    rec = cx.sample(pos0.clone(), t_arr, sc, nc, z, record=True)          # ... and the context is still usable
    assert bool(torch.isfinite(rec.pos).all())


def test_rigid_ligand_record_has_six_columns(dev):
    """n_rot = 0: the rows are [B, 6]; poses, scores and perturbations are recorded as for a flexible ligand"""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    c = synthetic.make_complex(8, n_res=40, n_lig=20)
    c['edge_mask'] = np.zeros_like(c['edge_mask'])
    c['mask_rotate'] = np.zeros((0, len(c['lig_pos'])), dtype=bool)
    ctx = Context(device=0)
    ctx.load_state_dict(smr.random_state_dict(CFG, seed=5))
    B, steps = 2, 3
    cx = Complex(ctx, c, B)
    _, t_arr, sc, nc = _coefficients(steps)
    pos0 = T(_pocket_poses(c, B, 4)).to(dev)
    z = (0.2 * torch.randn(steps, B, 6, generator=torch.Generator().manual_seed(1))).to(dev)
    pos = pos0.clone()
    rec = cx.sample(pos, t_arr, sc, nc, z, record=True)
    assert cx.R == 0 and tuple(rec.scores.shape) == tuple(rec.perturb.shape) == (steps, B, 6)
    assert torch.equal(rec.pos[0], pos0) and torch.equal(rec.pos[steps], pos)
    s, pt = rec.scores.cpu(), rec.perturb.cpu()
    assert bool(torch.isfinite(s).all()) and float(s.abs().min()) > 0
    col = torch.tensor([0, 0, 0, 1, 1, 1])
    host = T(sc)[:, col][:, None, :].double() * s.double() + T(nc)[:, col][:, None, :].double() * z.cpu().double()
    assert rel_err(pt, host) < 1e-6
    # a rigid step is an isometry of the ligand: pairwise distances stay
    d = lambda p: torch.cdist(p, p)
    assert rel_err(d(rec.pos[steps].cpu()), d(rec.pos[0].cpu())) < 1e-5


def test_no_torsion_record_has_zero_torsion_columns(dev):
    """a no_torsion context on a ligand WITH rotatable bonds: the rows keep the noise argument's layout 6 + n_rot, the torsion columns of scores and perturb are
    zero (whatever the noise array holds there), the ligand moves rigidly"""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    c = synthetic.make_complex(8, n_res=40, n_lig=20)
    ctx = Context(device=0, no_torsion=1)
    tor_keys = ('final_edge_embedding', 'tor_bond_conv', 'tor_final_layer')          # a no_torsion checkpoint has no torsion head
    ctx.load_state_dict({k: v for k, v in smr.random_state_dict(CFG, seed=5).items() if not k.startswith(tor_keys)})
    B, steps = 2, 3
    cx = Complex(ctx, c, B)
    assert cx.R > 0
    _, t_arr, sc, nc = _coefficients(steps)
    pos0 = T(_pocket_poses(c, B, 4)).to(dev)
    z = (0.2 * torch.randn(steps, B, 6 + cx.R, generator=torch.Generator().manual_seed(1))).to(dev)
    pos = pos0.clone()
    rec = cx.sample(pos, t_arr, sc, nc, z, record=True)
    assert tuple(rec.scores.shape) == (steps, B, 6 + cx.R)
    s, pt = rec.scores.cpu(), rec.perturb.cpu()
    assert float(s[:, :, 6:].abs().max()) == 0.0 and float(pt[:, :, 6:].abs().max()) == 0.0
    assert float(s[:, :, :6].abs().min()) > 0 and bool(torch.isfinite(pt).all())
    assert torch.equal(rec.pos[steps], pos)
    d = lambda p: torch.cdist(p, p)
    assert rel_err(d(rec.pos[steps].cpu()), d(rec.pos[0].cpu())) < 1e-5


class _Vis:
    """stand-in of utils/visualise.py's PDBFile: logs what sampling() adds"""

    def __init__(self, idx, log):
        self.idx, self.log, self.frames = idx, log, []

    def add(self, coords, part, order):
        assert not coords.is_cuda and (part, order) == (1, 2)
        self.log.append(self.idx)
        self.frames.append(coords.clone())


def test_sampling_visualization_list_and_trajectory(dev, golden):
    """sampling(visualization_list=..., trajectory=[]) on 4 graphs in 2 batches: no exception; as in utils/sampling.py:224-228 the WHOLE list is walked after
    every batch (8 calls, order 0 1 2 3 0 1 2 3); before its own batch has run a graph's frame is its start pose, the last frame of graph i is
    data_list[i]['ligand'].pos.cpu() + original_center; `trajectory` receives one record per batch whose pos[-1] equals the returned poses."""
    from helpers import complex_from_npz
    from test_gpu_model import ARGS_S, README_S, _ref_noise
    from disco_diffdock_amd.sampling import sampling
    from disco_diffdock_amd.model_utils import get_model
    from disco_diffdock_amd.data import from_arrays
    from disco_diffdock_amd.diffusion_utils import t_to_sigma, get_t_schedule
    tag = 'diffdockS_score_model'
    z, c = golden(f'trajectory_{tag}'), complex_from_npz(golden(f'complex_{tag}'))
    model = get_model(ARGS_S, dev, partial(t_to_sigma, args=ARGS_S), no_parallel=True)
    model.score_model.load_state_dict(smr.random_state_dict(CFG, seed=7), strict=True)
    N, bs, steps, n = 4, 2, 3, len(c['lig_pos'])
    R = int(c['edge_mask'].sum())
    rng = np.random.default_rng(0)
    dl = [from_arrays(c) for _ in range(N)]
    start = []
    for d in dl:
        d['ligand'].pos = T(z['pos0'][:n] + rng.normal(0, 1.0, size=(1, 3)).astype(np.float32))
        start.append(d['ligand'].pos.clone())
    center = dl[0].original_center.detach().cpu()
    sched = get_t_schedule(steps)
    noise = [_ref_noise(11 + b, steps, bs, R) for b in range(N // bs)]
    log, traj = [], []
    vis = [_Vis(i, log) for i in range(N)]
    out, conf = sampling(dl, model, steps, sched, sched, sched, dev, partial(t_to_sigma, args=ARGS_S), ARGS_S, batch_size=bs, no_final_step_noise=True,
                         use_latent=False, noise=noise, visualization_list=vis, trajectory=traj, **README_S)
    assert conf is None and log == list(range(N)) * (N // bs)
    for i, v in enumerate(vis):
        assert len(v.frames) == N // bs
        assert torch.equal(v.frames[-1], out[i]['ligand'].pos.cpu() + center)
        assert not torch.equal(out[i]['ligand'].pos.cpu(), start[i])
    for i in range(bs, N):          # graphs of the second batch: the first walk saw their start poses
        assert torch.equal(vis[i].frames[0], start[i] + center)
    assert len(traj) == N // bs
    for b, rec in enumerate(traj):
        assert rec.pos.is_cuda and tuple(rec.pos.shape) == (steps + 1, bs, n, 3) and tuple(rec.edge_counts.shape) == (steps, 4)
        ret = torch.stack([out[b * bs + i]['ligand'].pos for i in range(bs)])
        assert torch.equal(rec.pos[-1], ret)
        assert torch.equal(rec.pos[0].cpu(), torch.stack(start[b * bs:(b + 1) * bs]))
    # the same call without the two options returns the same poses (supplied noise; atomics leave ~1e-7 run-to-run noise)
    dl2 = [from_arrays(c) for _ in range(N)]
    for d, p in zip(dl2, start):
        d['ligand'].pos = p.clone()
    out2, _ = sampling(dl2, model, steps, sched, sched, sched, dev, partial(t_to_sigma, args=ARGS_S), ARGS_S, batch_size=bs, no_final_step_noise=True,
                       use_latent=False, noise=noise, **README_S)
    assert rel_err(torch.cat([d['ligand'].pos for d in out2]).cpu(), torch.cat([d['ligand'].pos for d in out]).cpu()) < 1e-5
