"""The score model's edge featurisation (csrc/k_graph.hip: graph_fill_kernel's edge lists, flipped-copy slots and deg; edge_features_body;
rec_edge_static_kernel) per EDGE against the oracle at fp64, on the adversarial classes of tests/adversarial_edges.py and at its bar (max(4 x err32,
8 x 2^-24 x scale); tests/test_edge_feature_bound.py shows on the host that the bar holds for a correct fp32 evaluation and that eight plausible slips
break it by orders of magnitude).  Every case is one forward and host copies of a few thousand edges.

What is compared: the edge multisets of the four groups (no edge is left out), every emb and sh row, deg against the exact in-degree, group 3 against group 1
bit for bit; with the receptive-field pruning on, everything but the rec-rec rows behind the level-C segment, whose number is asserted; with the cross mirror
off (one child process: the switch is read once per process), the cross classes again; for the latent-conditioned model also the shared rec-rec copy and the
per-sample patch group that layer 0 reads.  The all-atom confidence model's nine groups (csrc/conf.hip) are held to the same bar at the end.

Measured figures: profiles/r09_edge_feature_error.json, written by this module itself when DDK_EDGE_FEATURE_PROFILE names a file (every figure that check()
sees, plus - recorded, not asserted - the score-model figures under the reference that gets fp32 position tensors, adversarial_edges.reference(carry=False))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adversarial_edges as ae

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


def make_context(disco):
    from disco_diffdock_amd.runtime import Context
    ctx = Context(device=0, **(ae.CTX_DISCO if disco else {}))
    ctx.load_state_dict(ae.params(disco))
    return ctx


@pytest.fixture(scope='module')
def contexts(dev):
    made = {}

    def get(disco):
        if disco not in made:
            made[disco] = make_context(disco)
        return made[disco]
    yield get
    for ctx in made.values():
        ctx.set_pruning(True)
        ctx.close()


FIGURES = {}          # what -> {figure: dict(error, bar, err32, ...)}: everything check() and record() saw in this run


def record(fig, what):
    for k, (e, b, e32) in fig.items():
        FIGURES.setdefault(what, {})[f'{k[0]} {k[1]}'] = dict(error=float('%.4g' % e), err32=float('%.4g' % e32), bar=float('%.4g' % b),
                                                              error_over_err32=float('%.4g' % (e / e32)) if e32 else None, error_over_bar=float('%.4g' % (e / b)))


@pytest.fixture(scope='module', autouse=True)
def profile_file():
    """DDK_EDGE_FEATURE_PROFILE=<path>: the figures of this run as JSON (how profiles/r09_edge_feature_error.json is made)"""
    yield
    path = os.environ.get('DDK_EDGE_FEATURE_PROFILE')
    if path and FIGURES:
        ratios = [(v['error_over_err32'], w, k) for w, f in FIGURES.items() if 'fp32-tensor' not in w for k, v in f.items() if v['error_over_err32'] is not None]
        worst = {q: max((r for r in ratios if r[2].endswith(q)), default=None) for q in ('emb', 'sh')}
        about = ('Edge features on an MI355X against the oracle at fp64, per case, edge group and quantity: worst error over the group (emb: the output column with '
                 'the worst error / bar; sh: components / sqrt 3), err32 = the fp32 oracle\'s worst error there, bar = max(4 x err32, 8 x 2^-24 x scale).  Written by '
                 'tests/test_gpu_edge_features_adversarial.py under DDK_EDGE_FEATURE_PROFILE.  Entries marked [fp32-tensor reference] are measured against '
                 'adversarial_edges.reference(carry=False) and are not asserted.')
        with open(path, 'w') as f:
            json.dump(dict(_about=about, worst_error_over_err32={q: dict(ratio=w[0], case=w[1], figure=w[2]) for q, w in worst.items() if w},
                           worst_error_over_bar=max(v['error_over_bar'] for w, f_ in FIGURES.items() if 'fp32-tensor' not in w for v in f_.values()), cases=FIGURES), f, indent=1)


def forward(cs, ctx, prune, tails=False):
    """one score_forward of the case -> (graph_stats, [group] of dict(src, dst, emb, sh), deg, tails or None, whether the cross mirror wrote group 3)"""
    from disco_diffdock_amd.runtime import Complex
    dev = torch.device('cuda:0')
    ctx.set_pruning(prune)
    try:
        cx = Complex(ctx, cs.c, cs.B)
        if cs.disco:
            cx.set_latents(T(cs.lig_latent).to(dev), T(cs.rec_latent).to(dev), cs.unconditional)
        cx.score_forward(T(cs.pos).to(dev), cs.t, cs.t, cs.t)
        out = cx.read_edges(cs.B, tails=tails)
        mirror = cx.debug_cross_mirror()
    finally:
        ctx.set_pruning(True)
    st, src, dst, emb, sh, deg = out[:6]
    return st, ae.split_groups(st, src, dst, emb, sh), deg, (out[6] if tails else None), mirror


def check(fig, what):
    record(fig, what)
    for k, (e, b, e32) in fig.items():
        print(f'{what} {k[0]} {k[1]}: error {e:.3g} bar {b:.3g} err32 {e32:.3g} error/err32 {e / e32 if e32 else float("inf"):.2f}')
    assert not ae.broken(fig), (what, {k: fig[k] for k in ae.broken(fig)})


def mirror_is_bit_identical(got):
    o1, o3 = ae.mirror_pairs(got)
    return (np.array_equal(got[1]['emb'][o1].view(np.uint32), got[3]['emb'][o3].view(np.uint32))
            and np.array_equal(got[1]['sh'][o1].view(np.uint32), got[3]['sh'][o3].view(np.uint32)))


@pytest.mark.parametrize('name', ae.CLASSES)
def test_every_edge_row_is_within_the_bar(dev, contexts, name):
    """pruning off: all four groups complete.  Multisets, emb, sh, deg, and group 3 == group 1 bit for bit (the reference concatenates one tensor twice)"""
    cs = ae.case(name)
    st, got, deg, _, mirror = forward(cs, contexts(cs.disco), prune=False)
    r64 = ae.reference(cs)
    assert [len(g['src']) for g in got] == [len(g['src']) for g in r64]
    assert mirror          # these shapes fit the pair matrix: group 3 below IS the mirror path (the other path: test_cross_classes_with_the_mirror_off)
    check(ae.compare(cs, got), name)
    record(ae.compare(cs, got, carry=False), name + ' [fp32-tensor reference]')
    assert np.array_equal(deg, ae.in_degree(cs, r64))
    assert mirror_is_bit_identical(got)
    for g in got:
        assert bool((g['src'][1:] >= g['src'][:-1]).all())          # every group sorted by the receiving node
    if name == 'coincident':          # d = 0: sh is exactly [1, 0, 0, 0]
        n = cs.pos.shape[1]
        for i, j in cs.props['zero_ll']:
            m = (got[0]['src'] == i) & (got[0]['dst'] == j)
            assert m.sum() == 1 and np.array_equal(got[0]['sh'][m][0], [1, 0, 0, 0])
        i, j = cs.props['zero_lr']
        m = (got[1]['src'] == i) & (got[1]['dst'] == cs.B * n + j)
        assert m.sum() == 1 and np.array_equal(got[1]['sh'][m][0], [1, 0, 0, 0])


def test_pruning_on_exempts_only_the_rows_behind_the_level_c_segment(dev, contexts):
    """single_edge with the receptive-field pruning on: sample 0 has no cross edge (all its rec-rec edges are outside every level), sample 1 a single one.
    The rows before I_SEG + 3 are held to the bar; the rows behind it are the ONLY ones exempt, and there are exactly B * E_rr - (A + B + C) of them
    (graph_stats' E_rr_live is cumulative: levels A, A + B, A + B + C)."""
    cs = ae.case('single_edge')
    st, got, deg, _, mirror = forward(cs, contexts(False), prune=True)
    E_rr = cs.c['rec_edge_index'].shape[1]
    live = st['E_rr_live'][2]
    assert st['E_rr'] == cs.B * E_rr and st['E_rr_live'][0] <= st['E_rr_live'][1] <= live
    exempt = np.arange(cs.B * E_rr) >= live
    assert int(exempt.sum()) == cs.B * E_rr - live and E_rr <= int(exempt.sum()) < cs.B * E_rr          # at least all of sample 0, not everything
    check(ae.compare(cs, got, exempt=[None, None, exempt, None]), 'single_edge pruned')
    assert np.array_equal(deg, ae.in_degree(cs, ae.reference(cs))) and mirror_is_bit_identical(got)
    # the live segment holds whole receivers only: the rec-rec edges of the residues of levels A, B, C
    n_rec, nl = len(cs.c['rec_pos']), cs.B * cs.pos.shape[1]
    live_receivers, dead_receivers = set(got[2]['src'][~exempt].tolist()), set(got[2]['src'][exempt].tolist())
    assert not (live_receivers & dead_receivers) and all((r - nl) // n_rec != 0 for r in live_receivers)


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import numpy as np
import adversarial_edges as ae
import test_gpu_edge_features_adversarial as t
ctx = t.make_context(False)
for name in ae.CROSS_CLASSES:
    cs = ae.case(name)
    st, got, deg, _, mirror = t.forward(cs, ctx, prune=False)
    fig = ae.compare(cs, got)
    print('FIGURES ' + json.dumps(dict(name=name, mirror=bool(mirror), deg=bool(np.array_equal(deg, ae.in_degree(cs, ae.reference(cs)))), mirror_bits=bool(t.mirror_is_bit_identical(got)),
                                       figures={k[0] + ' ' + k[1]: [float(v) for v in f] for k, f in fig.items()})), flush=True)
'''


def test_cross_classes_with_the_mirror_off(dev):
    """DDK_NO_CROSS_MIRROR is read once into a static: one fresh child runs the cross classes with both directions evaluating their own features and prints the
    worst error and bar per group; asserted here.  That the switch took effect is read from the library (ddk_debug_cross_mirror: 0 in the child, 1 in this
    process, see test_every_edge_row_is_within_the_bar); the two directions run the same instructions on the same operands, so their rows still agree bit for bit."""
    env = dict(os.environ, DDK_NO_CROSS_MIRROR='1')
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [json.loads(l[len('FIGURES '):]) for l in r.stdout.splitlines() if l.startswith('FIGURES ')]
    assert [row['name'] for row in rows] == list(ae.CROSS_CLASSES)
    for row in rows:
        assert row['deg'] and len(row['figures']) == 8
        assert row['mirror'] is False and row['mirror_bits'] is True
        record({tuple(k.split()): v for k, v in row['figures'].items()}, row['name'] + ' [mirror off]')
        for k, (e, b, e32) in row['figures'].items():
            print(f'mirror off {row["name"]} {k}: error {e:.3g} bar {b:.3g} err32 {e32:.3g}')
            assert e <= b, (row['name'], k, e, b)


@pytest.mark.parametrize('u', [0, 1])
def test_disco_shared_copy_and_patch_group(dev, contexts, u):
    """latent-conditioned model: the one rec-rec copy layer 0 evaluates for the whole batch (sample 0's rows, ITS latents) and the per-sample patch group of
    the receivers that see a non-zero latent, each row against the reference row of the (sample, receiver, sender) it stands for, at group 2's bar"""
    cs = ae.case(f'latents_u{u}')
    ctx = contexts(True)
    st, got, deg, tail, mirror = forward(cs, ctx, prune=False, tails=True)
    if int(ctx.cfg.deterministic):          # the deterministic mode keeps the full evaluation: there IS no shared copy and no patch group to compare;
        assert st['E_shared'] == 0 and tail['shared'] is None and tail['patch'] is None          # what layer 0 reads instead, the four groups, is held to the bar
        check(ae.compare(cs, got), cs.name + ' [deterministic: no tails]')
        return
    r64, r32 = ae.references(cs)
    bars = ae.group_bars(r64[2], r32[2])
    n_rec, nl = len(cs.c['rec_pos']), cs.B * cs.pos.shape[1]
    ei = cs.c['rec_edge_index']
    E_rr = ei.shape[1]
    src, dst, emb, sh = tail['shared']
    assert st['E_shared'] == E_rr == len(src) and np.array_equal(src, nl + ei[0]) and np.array_equal(dst, nl + ei[1])          # sample 0's numbering, static order
    a = ae.lookup(cs, r64[2], src, dst)
    check({('shared ' + k, k): v for k, v in ae.hold(emb, sh, r64[2]['emb'][a], r64[2]['sh'][a], bars).items()}, cs.name)
    cnt, mask = tail['patch_counts'], tail['patch_mask']
    src, dst, emb, sh = tail['patch']
    outdeg = np.bincount(ei[0], minlength=n_rec)
    assert cnt[0] == 0 and not mask[0].any() and len(src) == cnt[cs.B] > 0
    marked = (np.abs(cs.rec_latent).sum(1) > 0).reshape(cs.B, n_rec)
    for b in range(1, cs.B):          # a receiver is patched iff it or one of its senders carries a latent in sample b or in sample 0
        mk = marked[b] | marked[0]
        want = mk.copy()
        np.logical_or.at(want, ei[0], mk[ei[1]])
        assert np.array_equal(mask[b].astype(bool), want) and cnt[b + 1] - cnt[b] == outdeg[want].sum()
        sl = slice(cnt[b], cnt[b + 1])
        assert ((src[sl] - nl) // n_rec == b).all() and ((dst[sl] - nl) // n_rec == b).all() and want[(src[sl] - nl) % n_rec].all()
    a = ae.lookup(cs, r64[2], src, dst)
    assert len(np.unique(a)) == len(a)
    check({('patch ' + k, k): v for k, v in ae.hold(emb, sh, r64[2]['emb'][a], r64[2]['sh'][a], bars).items()}, cs.name)


def test_confidence_model_nine_groups(dev):
    """all-atom confidence model: a set_atoms complex of 40 residues, 164 receptor atoms and 20 ligand atoms, B = 2 in a complex made for max_batch = 3 (so
    the device numbering, with its strides of max_batch and the virtual ligand-free sample, is not the oracle's).  After confidence_forward: the counts of
    all nine groups equal confidence_counts and the oracle's, every group's edge multiset equals the oracle's after the mapping, every emb and sh row is
    within the bar against confidence_ref's edge_sets, and the flipped groups al / rl / ra equal their forward groups' rows bit for bit."""
    from disco_diffdock_amd.runtime import Context, Complex
    cc = ae.conf_case()
    c, pos, Bm = cc['c'], cc['pos'], cc['max_batch']
    ctx = Context(device=0, all_atoms=1, embedding_scale=10000.0, num_confidence_outputs=2)
    ctx.load_state_dict(ae.conf_params())
    cx = Complex(ctx, c, max_batch=Bm)
    cx.set_atoms(c['atom_x'], c['atom_pos'], c['atom_edge_index'], c['atom_rec_index'])
    out = cx.confidence_forward(T(pos).to(dev))
    assert bool(torch.isfinite(out).all())
    counts, got = cx.confidence_counts(), cx.confidence_edges()
    ref = ae.conf_reference()
    assert {g: len(got[g][0]) for g in ae.CONF_GROUPS} == counts == {g: len(ref[g]['src']) for g in ae.CONF_GROUPS}
    assert min(counts.values()) > 0
    check(ae.conf_compare(got, Bm), 'confidence')
    for g in ae.CONF_FLIPPED:
        og, of = ae.conf_flipped_rows(got, g)
        f = ae.CONF_FLIPPED[g]
        assert np.array_equal(got[g][2][og].view(np.uint32), got[f][2][of].view(np.uint32)) and np.array_equal(got[g][3][og].view(np.uint32), got[f][3][of].view(np.uint32)), g
    ctx.close()
