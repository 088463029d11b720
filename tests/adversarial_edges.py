"""Adversarial geometry for the edge featurisation of the score model (csrc/k_graph.hip: edge_features_body, rec_edge_static_kernel, the flipped-copy
writes through e_aux, the deg array) and one case for the nine edge groups of the all-atom confidence model (csrc/conf.hip; conf_* below): seeded generators that return a small complex together with the properties they claim, the oracle's per-edge
features at fp64 and at fp32, the comparison that holds every edge row to the project's one bar, and a host restatement of the kernel in numpy fp32 with
named mutants.  Plain helper module (no fixtures, no GPU import): shared by tests/test_edge_feature_bound.py (CPU) and
tests/test_gpu_edge_features_adversarial.py.

THE BAR is adversarial_geometry.bar(err32, scale) = max(K * err32, FLOOR * scale), imported, not restated.  Per edge group and quantity:
    sh     the four components divided by sqrt 3, scale 1; err32 = the fp32 oracle's worst error over the group
    emb    per output column: scale = the largest |value| of that column over the group in the fp64 reference, err32 = the fp32 oracle's worst error in that
           column over the group; the figure reported for the group is the column with the worst error / bar
The references are oracle.score_model_ref.embed (with the conv stack switched off: num_conv_layers = 0) at fp64 and at fp32 ON THE SAME fp32 POSITIONS.
The fp64 one gets those fp32 values carried in fp64 tensors, so that the edge vector, its length, sh and the Gaussians' argument are fp64 evaluations too:
handing it fp32 tensors leaves the length an fp32 number in BOTH references, err32 then knows nothing of the one rounding that dominates the lig-lig
embeddings (an ulp of d = 3 A moves a Gaussian of the 5 A table by 4e-7; measured on the host restatement: 5 - 9 x err32 in group 0 from the kernel's own
correctly rounded d, 2 x err32 with torch's d copied bit for bit; the DEVICE under that variant, reference(carry=False): 8.6 x err32 = 2.2 x the bar in
lig-lig emb, 1.6 x the bar in the cross groups, recorded unasserted in profiles/r09_edge_feature_error.json), and the bar would ask for torch's bits instead of fp32's accuracy.  Carrying the
positions in fp64 could move a pair across a cutoff (the neighbour tests then run in fp64); reference() asserts that the fp64 edge lists ARE the fp32 ones,
and the generators keep their near-cutoff pairs 1e-5 (relative) inside, a hundred fp32 roundings.

Edges are matched by (group, src, dst); the device numbering [all ligand atoms | all residues] of a batch that fills the complex is the oracle's
(device_to_oracle checks it).  A bonded pair inside the radius is two rows of group 0 with the same key (the bond copy with its bond row, the radius copy
with a zero one): the two device rows are matched to the two reference rows by the better of the two assignments.

Not a supported input, and not generated: separations below one ulp of the coordinate (subnormal differences)."""
import dataclasses
import itertools

import numpy as np
import torch

from adversarial_geometry import K, bar, max_err
from helpers import batch_of
from oracle import sampler_ref as spr
from oracle import score_model_ref as smr

F32 = np.float32
SQRT3 = float(np.sqrt(3.0))
NS, DE, SIG = 24, 32, 32
CFG = smr.ScoreModelConfig(latent_vocab=64)
CFG_DISCO = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)
CTX_DISCO = dict(latent_dim=2, latent_vocab=1, latent_droprate=0.1)          # runtime.Context keywords of the latent-conditioned model
WEIGHT_SEED = 7
GROUPS = ('lig-lig', 'lig->rec', 'rec-rec', 'rec->lig')
TABLE = ('lig', 'cross', 'rec', 'cross')                                     # the Gaussian table / edge MLP of every group
CLASSES = ('coincident', 'binades', 'far_shift', 'far_mirror', 'bonded', 'cap', 'single_edge', 'latents_u0', 'latents_u1')
CROSS_CLASSES = ('coincident', 'binades', 'far_shift', 'single_edge')      # the classes the mirror-off run repeats (every way a cross edge is special)
MUTANTS = ('sh_negated_group3', 'sqrt3_omitted', 'bond_row_on_radius_copy', 'cross_table_for_lig', 'offsets_shifted', 'mirror_from_next_slot',
           'latent_columns_swapped', 'unconditional_always')
_cache = {}


@dataclasses.dataclass
class Case:
    name: str
    c: dict                      # the complex (numpy arrays in the layout runtime.Complex takes)
    pos: np.ndarray              # [B, n_lig, 3] float32
    t: float                     # diffusion time of the forward (sigma embedding, cross cutoff 3 sigma_tr + 20)
    props: dict                  # what the generator claims (tests/test_edge_feature_bound.py checks every entry)
    disco: bool = False
    lig_latent: np.ndarray = None          # [B * n_lig, 2] float32
    rec_latent: np.ndarray = None          # [B * n_rec, 2] float32
    unconditional: float = 0.0

    @property
    def B(self):
        return self.pos.shape[0]

    @property
    def cfg(self):
        return CFG_DISCO if self.disco else CFG


def params(disco=False):
    key = ('P', disco)
    if key not in _cache:
        _cache[key] = smr.random_state_dict(CFG_DISCO if disco else CFG, seed=WEIGHT_SEED)
    return _cache[key]


def cross_cutoff(t, cfg=CFG):
    return 3.0 * (cfg.tr_sigma_min ** (1 - t) * cfg.tr_sigma_max ** t) + 20.0


# ------------------------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------------------------
def _base(seed, n_res=48, n_lig=24):
    from disco_diffdock_amd import synthetic
    c = synthetic.make_complex(seed, n_res=n_res, n_lig=n_lig)
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _poses(c, B, rng, spread=1.0):
    return np.stack([c['lig_pos'].astype(np.float64) + rng.normal(0, spread, size=(1, 3)) for _ in range(B)]).astype(F32)


def _coincident():
    """B = 2.  In every sample: atoms 1 and 2 ON atom 0 (three coincident ligand atoms, d = 0 in six lig-lig edges), atom 3 one ulp of the x coordinate
    from atom 4, atom 5 ON residue 7 (a cross edge with d = 0), atom 6 one ulp of x from residue 8.  d = 0: reference F.normalize eps 1e-12, kernel
    fmaxf(d, 1e-12f), sh = [1, 0, 0, 0] in both.  Nothing below one ulp: subnormal separations are not a supported input."""
    c, rng = _base(31), np.random.default_rng(31)
    pos = _poses(c, 2, rng)
    up = lambda v: np.nextafter(v, F32(np.inf))
    for b in range(2):
        pos[b, 1] = pos[b, 2] = pos[b, 0]
        pos[b, 3] = pos[b, 4]
        pos[b, 3, 0] = up(pos[b, 4, 0])
        pos[b, 5] = c['rec_pos'][7]
        pos[b, 6] = c['rec_pos'][8]
        pos[b, 6, 0] = up(c['rec_pos'][8, 0])
    return Case('coincident', c, pos, 0.6, dict(zero_ll=[(0, 1), (0, 2), (1, 2)], ulp_ll=(3, 4), zero_lr=(5, 7), ulp_lr=(6, 8)))


def _binades():
    """B = 3, t = 1 (cross cutoff 77 A).  Pair distances across every Gaussian centre of the three tables that an edge can reach:
    lig (32 centres over 0..5 A)     samples 0 and 1: the atoms on a line at seeded positions in [0, 6] A - every centre has a pair within half a step
                                     below and above it, one pair sits 1e-5 inside the 5 A radius; bonds between line atoms up to 6 A long and, in sample
                                     2, tens of A long: beyond the last centre, every Gaussian underflows
    rec (32 centres over 0..30 A)    the last 18 of the 64 residues moved to 22.6, 23.1 .. 30.1, 60 and 100 A from residue 0 and joined to it by static edges in
                                     both directions, besides the receptor's own edges of 3.8..15 A and added edges (k, j) from residues k = 1..4 to every j: centres from
                                     3.9 A up (two residues are never closer than 3.8 A), and 60 / 100 A where exp(coeff t^2) underflows to 0
    cross (32 centres over 0..80 A)  sample 2: the atoms on a ray from residue 0, 0.05 .. 76.99 A from it (1e-5 inside the cutoff); with all the other
                                     residues that brackets every centre below the cutoff - the last two centres (77.4, 80 A) lie beyond any cross edge"""
    c, rng = _base(32, n_res=64), np.random.default_rng(32)
    n, n_rec = len(c['lig_pos']), len(c['rec_pos'])
    u = np.array([0.36, 0.48, 0.8])
    rp = c['rec_pos'].astype(np.float64)
    moved = list(range(n_rec - 18, n_rec))
    for j, d in zip(moved, [22.6 + 0.5 * k for k in range(16)] + [60.0, 100.0]):
        rp[j] = rp[0] + d * np.array([-0.6, 0.8, 0.0])
    c['rec_pos'] = rp.astype(F32)
    ei = c['rec_edge_index']
    extra = [(0, j) for j in moved] + [(j, 0) for j in moved] + [(k, j) for k in (1, 2, 3, 4) for j in range(n_rec) if j != k]
    have = set(zip(ei[0].tolist(), ei[1].tolist()))
    pairs = sorted(have | set(extra))          # grouped by source, as the library requires
    c['rec_edge_index'] = np.asarray(pairs, np.int64).T.copy()
    pocket = c['lig_pos'].mean(0).astype(np.float64)
    pos = np.zeros((3, n, 3))
    for b in range(2):
        x = np.sort(rng.uniform(0.0, 6.0, size=n))
        x[0], x[1] = 0.0, 0.02
        x[-1] = x[2] + 5.0 * (1 - 1e-5)
        if b == 1:          # one bond just beyond the last centre of the lig table (5.03 A: a bond copy without a radius copy, Gaussians not yet 0)
            i, j = c['bond_index'][:, 0]
            x[j] = x[i] + 5.03
        pos[b] = pocket + np.outer(x, u)
    d = np.concatenate([[0.05, 0.7], np.linspace(1.5, 74.0, n - 3), [77.0 * (1 - 1e-5)]])
    pos[2] = rp[0] + np.outer(d, u)
    return Case('binades', c, pos.astype(F32), 1.0, dict(ray_from=0, far_residues=(n_rec - 2, n_rec - 1), inside_cutoff_atom=n - 1))


def _far(kind):
    """B = 2.  far_shift: the whole complex (residues and both poses) moved by (150, -80, 60) A.  far_mirror: the whole complex mirrored through the origin
    and the ligand put across it, so that the coordinate differences of its edges change sign inside a sample."""
    c, rng = _base(33), np.random.default_rng(33)
    pos = _poses(c, 2, rng).astype(np.float64)
    rp = c['rec_pos'].astype(np.float64)
    if kind == 'far_shift':
        s = np.array([150.0, -80.0, 60.0])
        rp, pos = rp + s, pos + s
    else:
        pos = -(pos - pos.mean((0, 1)))          # the ligand centred on the origin: its atoms lie on both sides of every coordinate plane
        rp = -rp
    c['rec_pos'] = rp.astype(F32)
    return Case(kind, c, pos.astype(F32), 0.5, dict(max_abs_coordinate=float(np.abs(pos).max())))


def _bonded():
    """B = 2.  The ligand's own bonds (1.5 A: bond copy with aux >= 0 AND radius copy with a zero bond row in group 0) and two bonds stretched to 9 A by
    moving a leaf atom out (longer than the 5 A radius: the bond copy only).  bond_attr carries the generator's random one-hot types in all four columns."""
    c, rng = _base(34), np.random.default_rng(34)
    n = len(c['lig_pos'])
    bi = c['bond_index']
    degree = np.bincount(bi[0], minlength=n)
    leaves = [int(a) for a in np.where(degree == 1)[0]][:2]
    pos = _poses(c, 2, rng)
    cen = pos.mean(1)
    long_bonds = []
    for a in leaves:
        nb = int(bi[1][bi[0] == a][0])
        for b in range(2):
            out = pos[b, nb] - cen[b]
            pos[b, a] = pos[b, nb] + 9.0 * out / np.linalg.norm(out)
        long_bonds.append((a, nb))
    return Case('bonded', c, pos, 0.4, dict(long_bonds=long_bonds))


def _cap():
    """B = 2.  The compact 70-atom blob of test_neighbour_caps_bind_dense_ligand (a jittered 1.6 A grid: ~45 atoms within 5 A of an interior atom): the cap of
    32 neighbours binds, the kept neighbours are the first by index."""
    from disco_diffdock_amd import synthetic
    rng = np.random.default_rng(3)
    c = _base(12, n_res=40, n_lig=40)
    n = 70
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(4), indexing='ij'), -1).reshape(-1, 3)[:n] * 1.6
    pos = (g + rng.normal(0, 0.1, size=g.shape)).astype(F32)
    bonds = [(i, i + 1) for i in range(n - 1)]
    edge_mask, mask_rotate = synthetic.transformation_mask(n, bonds)
    ei = np.zeros((2, 2 * len(bonds)), np.int64)
    for k, (a, b) in enumerate(bonds):
        ei[:, 2 * k], ei[:, 2 * k + 1] = (a, b), (b, a)
    ea = np.zeros((2 * len(bonds), 4), F32)
    ea[np.arange(len(ea)), (np.arange(len(ea)) // 2) % 4] = 1
    c.update(lig_x=np.stack([rng.integers(0, d, size=n) for d in synthetic.LIG_FEATURE_DIMS], 1), lig_pos=pos, bond_index=ei, bond_attr=ea,
             edge_mask=edge_mask, mask_rotate=mask_rotate)
    return Case('cap', c, np.stack([pos, pos + F32(0.3)]), 0.7, dict(n=n, bonds=len(bonds)))


def _single_edge():
    """B = 3, t = 0.05 (cross cutoff 20.4 A).  Sample 0: the ligand 200 A away - an EMPTY cross graph, every residue outside the receptive field.  Sample 1:
    the ligand 200 A away except atom 0, which sits 1e-4 inside the cutoff of the outermost residue along a direction and outside every other residue's: ONE
    edge in group 1 and one in group 3.  Sample 2: an ordinary pose.  The third sample is there for the bar, not for the kernel: err32 and the column scale
    are maxima over a group, and over a group of one row they are luck (on this input the fp32 oracle is 6e-10 off in a column whose value is 5e-3, an
    honest fp32 chain 2e-8); the empty and the one-edge sample keep every offset path - an empty run, a run of one, a prefix over an empty sample."""
    c, rng = _base(35), np.random.default_rng(35)
    t = 0.05
    pos = _poses(c, 3, rng).astype(np.float64)
    pos[:2] += np.array([200.0, 0.0, 0.0])
    rp = c['rec_pos'].astype(np.float64)
    u = np.array([0.0, 0.6, 0.8])
    j = int(np.argmax(rp @ u))
    pos[1, 0] = rp[j] + u * cross_cutoff(t) * (1 - 1e-4)
    return Case('single_edge', c, pos.astype(F32), t, dict(residue=j, atom=0))


def _latents(unconditional):
    """B = 3, the DisCo configuration (latent_dim 2, latent_droprate 0.1).  Non-zero latents on a few nodes: one-hot picks as the AR model writes them and
    two rows with general values in both columns; sample 0 carries a receptor latent too (the shared rec-rec copy runs on ITS rows), sample 2 only ligand
    ones.  unconditional = 0 or 1 for the whole batch."""
    c, rng = _base(36), np.random.default_rng(36)
    B, n, n_rec = 3, len(c['lig_pos']), len(c['rec_pos'])
    ll, lr = np.zeros((B * n, 2), F32), np.zeros((B * n_rec, 2), F32)
    lr[0 * n_rec + 5, 0] = 1
    lr[1 * n_rec + 11, 1] = 1
    lr[1 * n_rec + 30] = (0.5, -1.25)
    ll[0 * n + 2, 1] = 1
    ll[1 * n + 7] = (-0.75, 2.0)
    ll[2 * n + 3, 0] = 1
    return Case(f'latents_u{int(unconditional)}', c, _poses(c, B, rng), 0.5, dict(rec_latent_nodes=[5, n_rec + 11, n_rec + 30], lig_latent_nodes=[2, n + 7, 2 * n + 3]),
                disco=True, lig_latent=ll, rec_latent=lr, unconditional=float(unconditional))


def case(name):
    if name not in _cache:
        make = dict(coincident=_coincident, binades=_binades, far_shift=lambda: _far('far_shift'), far_mirror=lambda: _far('far_mirror'), bonded=_bonded,
                    cap=_cap, single_edge=_single_edge, latents_u0=lambda: _latents(0), latents_u1=lambda: _latents(1))
        _cache[name] = make[name]()
    return _cache[name]


# ------------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------------
def reference(cs, dtype=torch.float64, carry=True):
    """oracle.score_model_ref.embed on the fp32 positions with the parameters and the arithmetic in `dtype` -> [group] of dict(src, dst, emb [E, 24], sh [E, 4])
    in numpy float64, the oracle's edge order inside a group.  Computed once per (case, dtype) and shared; callers must not write into it.
    carry=False hands embed the positions as fp32 TENSORS whatever `dtype` is (the edge length and sh stay fp32 evaluations: module docstring); no test
    holds anything to that variant, it exists so that the figures under it can be recorded beside the others."""
    key = ('ref', cs.name, dtype, carry)
    if key in _cache:
        return _cache[key]
    B = cs.B
    b = batch_of(cs.c, B, cs.pos)
    spr.set_time(b, cs.t, cs.t, cs.t, B)
    if cs.disco:
        b['ligand'].latent_h, b['receptor'].latent_h = torch.from_numpy(cs.lig_latent), torch.from_numpy(cs.rec_latent)
        b['ligand'].unconditional = torch.full((b['ligand'].num_nodes, 1), cs.unconditional)
        b['receptor'].unconditional = torch.full((b['receptor'].num_nodes, 1), cs.unconditional)
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params(cs.disco).items()}
    for nt in ('ligand', 'receptor'):          # the same fp32 VALUES, carried in `dtype`: the edge vector, its length and sh are evaluated in `dtype` too
        b[nt].pos = b[nt].pos.to(dtype if carry else torch.float32)
    g = smr.embed(P, dataclasses.replace(cs.cfg, num_conv_layers=0), b, dtype=dtype, return_graph=True)[-1]
    ei, (s1, s2, s3) = g['edge_index'].numpy(), g['splits']
    bounds = [0, s1, s2, s3, ei.shape[1]]
    out = []
    for k in range(4):
        sl = slice(bounds[k], bounds[k + 1])
        out.append(dict(src=ei[0, sl].astype(np.int64), dst=ei[1, sl].astype(np.int64), emb=g['edge_emb'][sl].double().numpy(), sh=g['edge_sh'][sl].double().numpy()))
    if dtype != torch.float32:          # the two references must stand on ONE edge set, the one fp32 neighbour tests give (module docstring)
        r32 = reference(cs, torch.float32)
        assert all(np.array_equal(a['src'], b_['src']) and np.array_equal(a['dst'], b_['dst']) for a, b_ in zip(out, r32)), \
            f'{cs.name}: a pair sits within fp32 rounding of a cutoff - the fp64 and the fp32 neighbour tests disagree'
    _cache[key] = out
    return out


def references(cs, carry=True):
    return reference(cs, torch.float64, carry), reference(cs, torch.float32, carry)


def n_nodes(cs):
    return cs.B * (len(cs.c['lig_pos']) + len(cs.c['rec_pos']))


def device_to_oracle(cs, node, max_batch=None):
    """device node ids -> the oracle's.  Both number [all ligand atoms | all residues] sample-major with the residues behind B * n_lig ligand atoms, so for
    the batch of a forward this is the identity; asserted, so that a change of either numbering fails here and not as a feature mismatch."""
    node = np.asarray(node, np.int64)
    assert node.size == 0 or (node.min() >= 0 and node.max() < n_nodes(cs)), 'node id outside [all ligand atoms | all residues] of the batch'
    return node


def in_degree(cs, ref):
    """the scatter-mean divisor per node: edges of all four groups received at the node (edge_index[0], tensor_layers.py:159)"""
    return np.bincount(np.concatenate([g['src'] for g in ref]), minlength=n_nodes(cs))


def split_groups(st, src, dst, emb, sh):
    """the device's merged edge arrays -> [group] of dict(src, dst, emb, sh) by the group counts of graph_stats()"""
    off = np.cumsum([0, st['E_ll'], st['E_lr'], st['E_rr'], st['E_rl']])
    assert off[4] == st['E'] == len(src)
    return [dict(src=src[off[k]:off[k + 1]], dst=dst[off[k]:off[k + 1]], emb=emb[off[k]:off[k + 1]], sh=sh[off[k]:off[k + 1]]) for k in range(4)]


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def group_bars(r64, r32):
    """per group: the bars of emb per column and of sh, from the two references alone -> dict(emb_bar [24], emb_err32 [24], sh_bar, sh_err32)"""
    if len(r64['src']) == 0:
        return dict(emb_bar=np.zeros(NS), emb_err32=np.zeros(NS), sh_bar=bar(0.0, 1.0), sh_err32=0.0)
    e32 = np.abs(r32['emb'] - r64['emb']).max(0)
    scale = np.abs(r64['emb']).max(0)
    s32 = max_err(r32['sh'] / SQRT3, r64['sh'] / SQRT3)
    return dict(emb_bar=np.array([bar(e, s) for e, s in zip(e32, scale)]), emb_err32=e32, sh_bar=bar(s32, 1.0), sh_err32=s32)


def hold(emb, sh, ref_emb, ref_sh, bars):
    """rows against their reference rows -> {'emb': (error, bar, err32), 'sh': (error, bar, err32)}: for emb the column with the worst error / bar (a
    non-finite value anywhere is an infinite error)"""
    if len(emb) == 0:
        return dict(emb=(0.0, float(bars['emb_bar'].min()), 0.0), sh=(0.0, bars['sh_bar'], bars['sh_err32']))
    d = np.abs(np.asarray(emb, np.float64) - ref_emb)
    err = np.where(np.isfinite(d).all(0), d.max(0), np.inf)
    col = int(np.argmax(err / bars['emb_bar']))
    return dict(emb=(float(err[col]), float(bars['emb_bar'][col]), float(bars['emb_err32'][col])),
                sh=(max_err(np.asarray(sh, np.float64) / SQRT3, ref_sh / SQRT3), bars['sh_bar'], bars['sh_err32']))


def _keys(cs, g):
    return device_to_oracle(cs, g['src']) * n_nodes(cs) + device_to_oracle(cs, g['dst'])


def align(cs, got, ref):
    """-> index array a with ref rows [a] standing for the rows of `got`, one group.  Asserts that the two edge MULTISETS are equal: no edge of either side
    is left out.  Rows that share a key (the bond copy and the radius copy of a bonded pair) take the assignment with the smaller worst emb difference."""
    return align_keys(_keys(cs, got), _keys(cs, ref), got['emb'], ref['emb'])


def align_keys(kg, kr, got_emb, ref_emb):
    """align() on ready-made integer keys of the two sides"""
    og, orf = np.argsort(kg, kind='stable'), np.argsort(kr, kind='stable')
    assert len(kg) == len(kr) and np.array_equal(kg[og], kr[orf]), 'edge multisets differ'
    a = np.empty(len(kg), np.int64)
    a[og] = orf
    ks = kg[og]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    for s, e in zip(start, np.r_[start[1:], len(ks)]):
        if e - s > 1:
            rows, cand = og[s:e], orf[s:e]
            assert e - s <= 3, 'more than three copies of one edge'
            cost = lambda perm: max(max_err(got_emb[r], ref_emb[p]) for r, p in zip(rows, perm))
            a[rows] = min(itertools.permutations(cand), key=cost)
    return a


def compare(cs, got, exempt=None, carry=True):
    """The per-edge contract.  got: [group] of dict(src, dst, emb, sh) in any order inside a group.  -> {(group name, 'emb' | 'sh'): (error, bar, err32)}
    over EVERY edge (the multisets are asserted equal), except the rows of exempt[group] (boolean per row of got; their edges still count in the multiset)."""
    r64, r32 = references(cs, carry)
    fig = {}
    for k, name in enumerate(GROUPS):
        a = align(cs, got[k], r64[k])
        assert np.array_equal(r64[k]['src'], r32[k]['src']) and np.array_equal(r64[k]['dst'], r32[k]['dst'])
        keep = np.ones(len(a), bool) if exempt is None or exempt[k] is None else ~np.asarray(exempt[k], bool)
        f = hold(got[k]['emb'][keep], got[k]['sh'][keep], r64[k]['emb'][a[keep]], r64[k]['sh'][a[keep]], group_bars(r64[k], r32[k]))
        fig[(name, 'emb')], fig[(name, 'sh')] = f['emb'], f['sh']
    return fig


def lookup(cs, ref_group, src, dst):
    """rows of one reference group that stand for the edges (src, dst) in device numbering (every key must exist exactly once: rec-rec edges)"""
    kr = _keys(cs, ref_group)
    o = np.argsort(kr)
    k = device_to_oracle(cs, src) * n_nodes(cs) + device_to_oracle(cs, dst)
    i = np.searchsorted(kr[o], k)
    assert len(np.unique(kr)) == len(kr) and (i < len(kr)).all() and np.array_equal(kr[o][i], k), 'an edge without a reference row'
    return o[i]


def broken(fig):
    return [k for k, (e, b, _) in fig.items() if not e <= b]


def ratio(err, the_bar):
    """error in units of the bar's own err32 term: K * err / bar, so a figure of K sits on the bar"""
    return float(K * err / the_bar)


def mirror_pairs(got):
    """-> (rows of group 1, rows of group 3) of the same (ligand atom, residue) pairs, in the same order"""
    n = int(max(got[1]['src'].max(initial=0), got[3]['dst'].max(initial=0), got[1]['dst'].max(initial=0), got[3]['src'].max(initial=0))) + 1
    k1 = got[1]['src'].astype(np.int64) * n + got[1]['dst']
    k3 = got[3]['dst'].astype(np.int64) * n + got[3]['src']
    o1, o3 = np.argsort(k1, kind='stable'), np.argsort(k3, kind='stable')
    assert np.array_equal(k1[o1], k3[o3]) and len(np.unique(k1)) == len(k1)
    return o1, o3


# ------------------------------------------------------------------------------------------------------------------------------------
# the all-atom confidence model (csrc/conf.hip): nine edge groups
# ------------------------------------------------------------------------------------------------------------------------------------
CONF_GROUPS = ('ll', 'lr', 'la', 'aa', 'al', 'ar', 'rr', 'rl', 'ra')          # runtime.CONF_GROUPS: the order of the device's group tables
CONF_FLIPPED = dict(al='la', rl='lr', ra='ar')                                  # a flipped group carries its forward group's rows (all_atom_score_model.py:245-258)
CONF_SEED = 5


def conf_case():
    """-> dict(c, pos [2, n_lig, 3] float32, max_batch = 3): a set_atoms complex of 40 residues, ~150 receptor atoms (3 - 5 per residue) and ~20 ligand atoms,
    two poses in a pocket (the centred ligand on a receptor atom, 1 A jitter: ligand-atom edges within 5 A exist in both).  max_batch is one more than the
    batch, so the device's node numbering (strides of max_batch, the virtual ligand-free sample behind the real ones) is NOT the oracle's."""
    if 'conf_case' not in _cache:
        from disco_diffdock_amd import synthetic
        c = _base(41, n_res=40, n_lig=20)
        rng = np.random.default_rng(41)
        synthetic.add_receptor_atoms(c, rng, atoms_per_residue=(3, 5))
        lig0 = c['lig_pos'].astype(np.float64) - c['lig_pos'].mean(0, keepdims=True)
        pos = np.stack([lig0 + c['atom_pos'][17] + rng.normal(0, 1.0, size=(1, 3)) for _ in range(2)]).astype(F32)
        _cache['conf_case'] = dict(c=c, pos=pos, max_batch=3)
    return _cache['conf_case']


def conf_params():
    from oracle import confidence_ref as cr
    if 'conf_P' not in _cache:
        _cache['conf_P'] = cr.random_state_dict(cr.ConfidenceModelConfig(), seed=CONF_SEED)
    return _cache['conf_P']


def conf_reference(dtype=torch.float64):
    """oracle.confidence_ref.confidence_forward(return_intermediates=True) without its conv stack (stop_after = 0), parameters and arithmetic in `dtype`, the
    fp32 positions carried in `dtype` as for the score model -> {group: dict(src, dst, emb, sh [E, 4])} for all nine groups, type-local node indices (the
    oracle's: ligand atom b * n_lig + i, receptor atom b * n_atom + a, residue b * n_rec + r).  The oracle's sh has nine components (lmax = 2); the device
    stores the first four and forms the l = 2 ones inside the conv kernel, so four are compared."""
    key = ('conf_ref', dtype)
    if key in _cache:
        return _cache[key]
    from helpers import to_graph
    from oracle import confidence_ref as cr
    from oracle import graph_lite
    cc = conf_case()
    c, pos, B = cc['c'], cc['pos'], cc['pos'].shape[0]
    b = graph_lite.collate([graph_lite.add_atoms(to_graph(c), c['atom_x'], c['atom_pos'], c['atom_edge_index'], c['atom_rec_index']) for _ in range(B)])
    b['ligand'].pos = torch.from_numpy(pos.reshape(-1, 3))
    for nt in ('ligand', 'receptor', 'atom'):
        b[nt].node_t = {k: torch.zeros(b[nt].num_nodes) for k in ('tr', 'rot', 'tor')}
        b[nt].pos = b[nt].pos.to(dtype)
    b.complex_t = {k: torch.zeros(B) for k in ('tr', 'rot', 'tor')}
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in conf_params().items()}
    _, inter = cr.confidence_forward(P, cr.ConfidenceModelConfig(), b, dtype=dtype, return_intermediates=True, stop_after=0)
    out = {}
    for g in CONF_GROUPS:
        ei, emb, sh = inter['edge_sets'][CONF_FLIPPED.get(g, g)]
        ei = ei.numpy().astype(np.int64)
        src, dst = (ei[1], ei[0]) if g in CONF_FLIPPED else (ei[0], ei[1])
        out[g] = dict(src=src, dst=dst, emb=emb.double().numpy(), sh=sh[:, :4].double().numpy())
    if dtype != torch.float32:
        r32 = conf_reference(torch.float32)
        assert all(np.array_equal(out[g]['src'], r32[g]['src']) and np.array_equal(out[g]['dst'], r32[g]['dst']) for g in CONF_GROUPS), \
            'confidence case: the fp64 and the fp32 neighbour tests disagree about a pair'
    _cache[key] = out
    return out


def conf_device_to_oracle(node, kind, B, max_batch, n_lig, n_atom, n_rec):
    """device node ids of one node type ('l', 'a', 'r') -> the oracle's type-local index.  Device: [ligand b * n_lig + i | atom Bm * n_lig + b * n_atom + a |
    residue Bm * n_lig + (Bm + 1) * n_atom + b * n_rec + r] with Bm = max_batch and atom / residue sample Bm the virtual ligand-free one, which no edge
    of the full group table may name."""
    node = np.asarray(node, np.int64)
    base = dict(l=0, a=max_batch * n_lig, r=max_batch * n_lig + (max_batch + 1) * n_atom)[kind]
    per = dict(l=n_lig, a=n_atom, r=n_rec)[kind]
    local = node - base
    assert node.size == 0 or (local.min() >= 0 and local.max() < B * per), f'a {kind} node id outside the {B} real samples'
    return local


def conf_compare(got, max_batch):
    """got: runtime.Complex.confidence_edges() = {group: (src, dst, emb, sh)} in device numbering -> {(group, 'emb' | 'sh'): (error, bar, err32)} for all nine
    groups; the edge multisets are asserted equal (no edge left out)"""
    cc = conf_case()
    c, B = cc['c'], cc['pos'].shape[0]
    n_lig, n_atom, n_rec = len(c['lig_pos']), len(c['atom_pos']), len(c['rec_pos'])
    r64, r32 = conf_reference(torch.float64), conf_reference(torch.float32)
    big = B * max(n_lig, n_atom, n_rec)
    fig = {}
    for g in CONF_GROUPS:
        src, dst, emb, sh = got[g]
        ks = conf_device_to_oracle(src, g[0], B, max_batch, n_lig, n_atom, n_rec) * big + conf_device_to_oracle(dst, g[1], B, max_batch, n_lig, n_atom, n_rec)
        a = align_keys(ks, r64[g]['src'] * big + r64[g]['dst'], emb, r64[g]['emb'])
        f = hold(emb, sh, r64[g]['emb'][a], r64[g]['sh'][a], group_bars(r64[g], r32[g]))
        fig[(g, 'emb')], fig[(g, 'sh')] = f['emb'], f['sh']
    return fig


def conf_flipped_rows(got, g):
    """-> (rows of the flipped group g, rows of its forward group) of the same pairs in the same order"""
    f = CONF_FLIPPED[g]
    n = int(max(got[g][0].max(initial=0), got[g][1].max(initial=0), got[f][0].max(initial=0), got[f][1].max(initial=0))) + 1
    kf = got[f][0].astype(np.int64) * n + got[f][1]
    kg = got[g][1].astype(np.int64) * n + got[g][0]
    og, of = np.argsort(kg, kind='stable'), np.argsort(kf, kind='stable')
    assert np.array_equal(kg[og], kf[of]) and len(np.unique(kf)) == len(kf)
    return og, of


# ------------------------------------------------------------------------------------------------------------------------------------
# the host restatement of edge_features_body / rec_edge_static_kernel
# ------------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64, the sum is rounded once to fp64 and once to fp32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _exp32(x):
    """the correctly rounded fp32 exponential (numpy's own fp32 exp is an ulp off at six of the sixteen frequencies of the sigma embedding, which moves the
    sines by 1e-5 and the embeddings by 1e-6; torch's and the C library's are correctly rounded there)"""
    return np.exp(np.asarray(x, F32).astype(np.float64)).astype(F32)


def _tables(cs):
    """the kernel's operands from the checkpoint, as model.hip packs them: per table offset, coeff, w1d [24, 32], w1b / w1l, w2, b2, unc and the
    per-forward sigb = b1 + W1[:, sigma columns] . sinusoidal(embedding_scale * t) in fp32, sequentially"""
    P, cfg, ld = params(cs.disco), cs.cfg, cs.cfg.latent_dim
    half = SIG // 2
    e = np.log(10000.0) / (half - 1)
    f = _exp32(np.arange(half, dtype=F32) * F32(-e))
    a = (F32(F32(cfg.embedding_scale) * F32(cs.t)) * f).astype(np.float64)          # (an ulp of these frequencies is 4e-5 rad at 1000 t = 600: see _exp32)
    sig = np.concatenate([np.sin(a), np.cos(a)]).astype(F32)
    out = {}
    for tab, nb in (('lig', 4), ('rec', 0), ('cross', 0)):
        W1 = P[f'{tab}_edge_embedding.0.weight'].numpy().astype(F32)
        sigb = P[f'{tab}_edge_embedding.0.bias'].numpy().astype(F32).copy()
        for k in range(SIG):
            sigb = (sigb + W1[:, nb + k] * sig[k]).astype(F32)
        off = P[f'{tab}_distance_expansion.offset'].numpy().astype(F32)
        d = float(off[1] - off[0])
        out[tab] = dict(offset=off, coeff=F32(-0.5 / (d * d)), step=off[1] - off[0], sigb=sigb, w1b=W1[:, :nb], w1d=W1[:, nb + SIG:nb + SIG + DE],
                        w1l=W1[:, nb + SIG + DE:nb + SIG + DE + 2 * ld], w2=P[f'{tab}_edge_embedding.3.weight'].numpy().astype(F32),
                        b2=P[f'{tab}_edge_embedding.3.bias'].numpy().astype(F32),
                        unc=P[f'{tab}_edge_unconditional_embedding'].numpy().astype(F32).reshape(-1) if cfg.latent_droprate > 0 else None)
    return out


def host_edges(cs, mutant=None):
    """edge_features_body (and rec_edge_static_kernel + the host's rr_sh for group 2) restated in numpy fp32 in source order, on the edge lists of the fp32
    reference -> [group] of dict(src, dst, emb, sh) float32.  `mutant` names one deliberate error (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS
    ref = reference(cs, torch.float32)
    T = _tables(cs)
    B, n_lig, n_rec = cs.B, len(cs.c['lig_pos']), len(cs.c['rec_pos'])
    nl = B * n_lig
    lp, rp = cs.pos.reshape(-1, 3).astype(F32), np.asarray(cs.c['rec_pos'], F32)
    M = cs.c['bond_index'].shape[1]
    ba = np.asarray(cs.c['bond_attr'], F32)
    bonded = set(zip(cs.c['bond_index'][0].tolist(), cs.c['bond_index'][1].tolist()))
    out = []
    for g in range(4):
        src, dst = ref[g]['src'], ref[g]['dst']
        E = len(src)
        tab = T['cross' if (g == 0 and mutant == 'cross_table_for_lig') else TABLE[g]]
        mlp = T[TABLE[g]]
        if g == 0:
            v = lp[dst] - lp[src]
        elif g == 2:
            v = rp[(dst - nl) % n_rec] - rp[(src - nl) % n_rec]
        else:
            li, ri = (src, dst) if g == 1 else (dst, src)
            v = rp[(ri - nl) % n_rec] - lp[li]
        vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
        d = np.sqrt(vx * vx + vy * vy + vz * vz, dtype=F32)
        inv = (F32(1.0) if mutant == 'sqrt3_omitted' else F32(1.7320508075688772)) / np.maximum(d, F32(1e-12))
        sh = np.stack([np.ones(E, F32), vx * inv, vy * inv, vz * inv], 1).astype(F32)
        if g == 3 and mutant == 'sh_negated_group3':
            sh[:, 1:] = -sh[:, 1:]
        offset = tab['offset'] + (tab['step'] if mutant == 'offsets_shifted' else F32(0))
        with np.errstate(under='ignore'):
            tt = d[:, None] - offset[None, :]
            gs = _exp32(tab['coeff'] * (tt * tt))
        if g == 2:          # rec_edge_static_kernel: a2 += w1d[o][q] * gs[q] from zero, then + sigb in the feature kernel
            h = np.zeros((E, NS), F32)
            for q in range(DE):
                h = (h + mlp['w1d'][None, :, q] * gs[:, q:q + 1]).astype(F32)
            h = (h + mlp['sigb'][None]).astype(F32)
        else:
            h = np.broadcast_to(mlp['sigb'][None], (E, NS)).astype(F32)
            for q in range(DE):
                h = _fma(mlp['w1d'][None, :, q], gs[:, q:q + 1], h)
        if g == 0:          # the oracle lists the B * M bond copies first, then the radius copies
            aux = np.full(E, -1, np.int64)
            aux[:B * M] = np.tile(np.arange(M), B)
            if mutant == 'bond_row_on_radius_copy':
                lookup_m = {p: m for m, p in enumerate(zip(cs.c['bond_index'][0].tolist(), cs.c['bond_index'][1].tolist()))}
                for e in range(B * M, E):
                    p = (int(src[e] % n_lig), int(dst[e] % n_lig))
                    if p in bonded:
                        aux[e] = lookup_m[p]
            w, rows = mlp['w1b'], ba[np.maximum(aux, 0)]
            add = (w[None, :, 0] * rows[:, 0:1] + w[None, :, 1] * rows[:, 1:2] + w[None, :, 2] * rows[:, 2:3] + w[None, :, 3] * rows[:, 3:4]).astype(F32)
            h = np.where((aux >= 0)[:, None], (h + add).astype(F32), h)
        if cs.disco and g in (0, 2):
            lat, off_, ld = (cs.lig_latent, 0, 2) if g == 0 else (cs.rec_latent, nl, 2)
            a, b_ = (dst, src) if mutant == 'latent_columns_swapped' else (src, dst)
            for j in range(ld):
                ls, ldv = lat[a - off_, j:j + 1], lat[b_ - off_, j:j + 1]
                h = (h + (mlp['w1l'][None, :, j] * ls + mlp['w1l'][None, :, ld + j] * ldv).astype(F32)).astype(F32)
        h = np.maximum(h, F32(0))
        y = np.broadcast_to(mlp['b2'][None], (E, NS)).astype(F32)
        for k in range(NS):
            y = _fma(mlp['w2'][None, :, k], h[:, k:k + 1], y)
        uncw = F32(0)
        if cs.disco and mlp['unc'] is not None:
            uncw = F32(1.0 if mutant == 'unconditional_always' else cs.unconditional)
        if uncw != 0:
            y = (y + uncw * mlp['unc'][None]).astype(F32)
        out.append(dict(src=src, dst=dst, emb=y, sh=sh))
    if mutant == 'mirror_from_next_slot' and len(out[3]['src']) > 1:      # the flipped copy lands one slot on in the (residue, atom) order of group 3
        o = np.lexsort((out[3]['dst'], out[3]['src']))
        for q in ('emb', 'sh'):
            rolled = out[3][q].copy()
            rolled[o] = out[3][q][np.roll(o, 1)]
            out[3][q] = rolled
    return out
