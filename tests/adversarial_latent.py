"""Adversarial cases for the kernels that make or feed the DisCo path's one discrete decision per graph and latent dimension - which node carries the
latent: gumbel_fwd_kernel / gumbel_bwd_kernel (csrc/k_gumbel.hip), ar_decode_kernel and ar_logits_kernel (csrc/k_ar.hip).  Seeded generators that return
their inputs together with the properties they claim, and plain numpy references.  Plain helper module (no fixtures, no GPU import): shared by
tests/test_latent_choice_host.py (CPU: the claims hold, the references agree with the oracle's) and tests/test_gpu_latent_choice_adversarial.py.

A wrong pick is still a valid one-hot, so nothing downstream notices it: every case here either has its expectation BY CONSTRUCTION (exact ties, saturated
logits, integer sums) or carries a margin, checked on the CPU, that the device's arithmetic cannot cross.

The Gumbel references are tests/latent_embedding_ref.py's (gumbel_uniforms, gumbel_noise, gumbel_forward, gumbel_backward); nothing of them is restated."""
import numpy as np

import latent_embedding_ref as lref

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# ------------------------------------------------------------------------------------------------------------------------------------
# the Gumbel softmax: one workgroup of RAGGED_T threads (csrc/k_ragged.h; GUM_T here) per (graph, d); thread t owns the quads t, t + RAGGED_T, ... of four positions each
# ------------------------------------------------------------------------------------------------------------------------------------
GUM_T, QUAD = 256, 4
GUMBEL_SEED, GUMBEL_SAMPLE, GUMBEL_DRAW = 0x1234567890ABCDEF, 3, 17
D_MAX = 4
BIG = F32(1e30)                      # a logit the noise cannot move: ulp(1e30f) = 7.6e22 in fp32, 1.4e14 in fp64
TWO_TRIPS = ((300, 1500), (0, 1025), (1, 0), (0, 0), (1024, 0), (3, 6))
MARGIN_GUMBEL = 1e-4                 # the fp64 argmax margin of logit + gum that fp32 cannot flip (tests/test_gpu_gumbel.py asserts the same)
CASE_SEEDS = dict(two_trips=1, saturated_ties=2, flat=3)


def thread_trip(p):
    """position p of a graph -> (thread, trip) of the kernel's loops: quad q = p // 4 belongs to thread q % 256 on its trip q // 256"""
    q = int(p) // QUAD
    return q % GUM_T, q // GUM_T


def _streams(name, G):
    from disco_diffdock_amd.runtime import stream_id
    return [stream_id(f'adversarial_latent_{name}_{g}') for g in range(G)]


def _normal_tables(rng, graphs):
    """per graph [n, D_MAX] float32 standard normal, the ligand's nodes first; a case at D < D_MAX takes the first D columns, so that column d of a
    graph holds the same logits (and draws the same noise, which is keyed by d) at every D"""
    return [rng.standard_normal((nl + nr, D_MAX)).astype(F32) for nl, nr in graphs]


def gumbel_case(name, D=D_MAX):
    """-> dict(name, graphs [(n_lig, n_rec)], T, D, streams [G], logits / grads: per graph [n, D] float32, claims).  The cases:

    two_trips       graphs of 1800, 1025, 1, 0, 1024 and 9 nodes; 1025 leaves one position alone in thread 0's second quad, 1024 fills every thread exactly
                    once, the empty graph sits in the middle, two graphs have no ligand side.  T is the caller's (claims['T'] lists the two that are run).
    saturated_ties  T = 1, two graphs of (700, 500): logit 1e30f at {1029, 1000, 699, 700} in the first, at {1029, 1000} in the second.  1e30f + gum == 1e30f in
                    fp32 and in fp64 alike, so z ties EXACTLY on the device whatever the library's log returns: y is exactly 1 / k at the k tied positions and exactly 0 elsewhere, hard sits
                    at the lowest tied position.  claims: tied, hard, and for every tied position its (thread, trip).
    flat            T = 1e30, one graph of (5, 1100): every expf argument is within 1e-28 of 0, every exponential exactly 1, y exactly 1 / 1105 everywhere and hard
                    at position 0 - the all-way tie through the whole tree.  grad_out is 1e24 * normal, so that grad_logit = y (g - sum g y) / T is of the order of
                    1e-9 and not a run of numbers under elem_err's absolute 1e-30.
    sharp           T = 0.01, two_trips' first graph (same stream, same logits) with grad_out entries drawn from {1e-20, 1, 1e20} * normal."""
    if name not in ('two_trips', 'saturated_ties', 'flat', 'sharp'):
        raise ValueError(name)
    base = 'two_trips' if name == 'sharp' else name
    rng = np.random.default_rng(CASE_SEEDS[base])
    if base == 'two_trips':
        graphs = TWO_TRIPS
        logits, grads = _normal_tables(rng, graphs), _normal_tables(rng, graphs)
        streams = _streams(base, len(graphs))
        case = dict(T=None, claims=dict(T=(1.0, 0.01), alone_in_second_quad=(1, 1024), every_thread_once=4, empty=3, no_ligand=(1, 3), unique_maximum=True))
        if name == 'sharp':
            graphs, logits, streams = graphs[:1], logits[:1], streams[:1]
            n = sum(graphs[0])
            grads = [(np.random.default_rng(4).choice(np.array([1e-20, 1.0, 1e20]), size=(n, D_MAX)) * rng.standard_normal((n, D_MAX))).astype(F32)]
            case = dict(T=0.01, claims=dict(grad_scales=(1e-20, 1.0, 1e20), unique_maximum=True))
    elif base == 'saturated_ties':
        graphs = ((700, 500), (700, 500))
        logits, grads = _normal_tables(rng, graphs), _normal_tables(rng, graphs)
        tied = ((1029, 1000, 699, 700), (1029, 1000))
        for g, at in enumerate(tied):
            logits[g][list(at), :] = BIG
        streams = _streams(base, 2)
        case = dict(T=1.0, claims=dict(tied=tied, hard=(699, 1000), where={p: thread_trip(p) for p in tied[0]}, boundary=(699, 700), unique_maximum=False))
    else:
        graphs = ((5, 1100),)
        logits = _normal_tables(rng, graphs)
        grads = [(1e24 * rng.standard_normal((1105, D_MAX))).astype(F32)]
        streams = _streams(base, 1)
        case = dict(T=1e30, claims=dict(y=F32(1) / F32(1105), hard=0, unique_maximum=False))
    case.update(name=name, graphs=tuple(graphs), D=D, streams=streams, logits=[a[:, :D].copy() for a in logits], grads=[a[:, :D].copy() for a in grads])
    return case


def gumbel_uniforms(case, g, d):
    """the fp32 uniforms graph g of the case draws for latent dimension d (bit-exact host mirror)"""
    return lref.gumbel_uniforms(GUMBEL_SEED, case['streams'][g], GUMBEL_SAMPLE, GUMBEL_DRAW, d, sum(case['graphs'][g]))


def gumbel_margin(case, g, d):
    """fp64: (argmax of logit + gum, the gap of the two largest; inf for one node)"""
    z = case['logits'][g][:, d].astype(np.float64) + lref.gumbel_noise(gumbel_uniforms(case, g, d))
    top = np.sort(z)
    return int(np.argmax(z)), (float(top[-1] - top[-2]) if len(z) > 1 else float('inf'))


# ------------------------------------------------------------------------------------------------------------------------------------
# the AR pick
# ------------------------------------------------------------------------------------------------------------------------------------
AR_SIZES = ((7, 30), (19, 300), (40, 500))      # n = 37, 319, 540: a thread of ar_decode_kernel owns 1, 2, 3 logits; at 319 the threads from 160 on own none
AR_THREADS = 256
AR_ARGMAX_T = (100.0, 1e4)
AR_SAMPLE_T = 6.0
AR_MARGIN = 1e-5
AR_RANDOM_ROWS = 40
AR_SEEDS = {37: 11, 319: 12, 540: 13}


def ar_chunk(n):
    """logits per thread of ar_decode_kernel: thread t owns [t * per, min((t + 1) * per, n))"""
    return (n + AR_THREADS - 1) // AR_THREADS


def ar_pick_ref(logits_row, T, u=None):
    """The pick rule of ddk_ar_decode (include/ddk.h) on one row -> (index, margin).  The product logit * T is formed in fp32, as the kernel does.
    T >= 100: argmax in torch's order - NaN is the largest value, the first of equals wins; margin None.
    else: p = min(exp(float64(product)), FLT_MAX) with NaN -> 0, a sequential fp64 cumsum, the first index with cum > float64(u) * cum[-1], otherwise n - 1;
    margin = min_i |cum_i - target| / total (inf where the total is 0): how far the target is from every point where the pick changes."""
    lg = np.asarray(logits_row, F32)
    with np.errstate(all='ignore'):
        prod = lg * F32(T)
        if F32(T) >= F32(100.0):
            nan = np.isnan(prod)
            return (int(np.argmax(nan)) if nan.any() else int(np.argmax(prod))), None
        p = np.minimum(np.exp(prod.astype(np.float64)), FLT_MAX)
        p[np.isnan(p)] = 0.0
        cum = np.cumsum(p)      # (numpy's cumsum adds in sequence)
        total = cum[-1]
        target = np.float64(F32(u)) * total
        over = cum > target
        idx = int(np.argmax(over)) if over.any() else len(lg) - 1
        margin = float(np.abs(cum - target).min() / total) if total > 0 else float('inf')
    return idx, margin


def _fp32_below(x):
    """the largest fp32 that is <= x"""
    f = F32(x)
    return f if float(f) <= x else np.nextafter(f, F32(0))


def ar_decode_cases(n_lig, n_rec):
    """-> dict(argmax=[row], sample=[row]); row = dict(name, logits [n] float32, u (float32; sample rows only), expect, why).  One row is one graph of a
    ddk_ar_decode call; the argmax rows run at each temperature of AR_ARGMAX_T, the sample rows at AR_SAMPLE_T.  `expect` is by construction except for
    'negative' and the 'random' rows, whose expectation is ar_pick_ref's (tests/test_latent_choice_host.py checks that ar_pick_ref agrees on all of them)."""
    n, per = n_lig + n_rec, ar_chunk(n_lig + n_rec)
    rng = np.random.default_rng(AR_SEEDS[n])
    normal = lambda: rng.standard_normal(n).astype(F32)
    far = n_lig + (3 * n_rec) // 4
    arg, smp = [], []

    def row(rows, name, lg, expect, why, u=None):
        rows.append(dict(name=name, logits=np.asarray(lg, F32), u=None if u is None else F32(u), expect=int(expect), why=why))

    # ---- argmax ----
    for name, at in (('max_first', 0), ('max_last_ligand', n_lig - 1), ('max_first_residue', n_lig), ('max_last', n - 1)):
        lg = normal()
        lg[at] = 10.0
        row(arg, name, lg, at, 'a unique maximum')
    lg = normal()
    lg[[n_lig - 1, n_lig, far]] = 7.0
    row(arg, 'tie3', lg, n_lig - 1, 'a tie of three across the ligand/receptor boundary and two thread chunks: the lowest wins')
    row(arg, 'all_neg_inf', np.full(n, -np.inf), 0, 'all -inf picks node 0')
    lg = normal()
    lg[n_lig - 2], lg[far] = np.inf, np.nan
    row(arg, 'nan_after_inf', lg, far, 'NaN counts as the largest value')
    lg = normal()
    lg[n_lig + 1], lg[n - 2] = np.nan, np.nan
    row(arg, 'two_nans', lg, n_lig + 1, 'the first of two NaNs')
    lg = normal()
    lg[n_lig], lg[far], lg[n - 1] = 1e37, 3e37, 2e37
    row(arg, 'overflow', lg, n_lig, 'products that overflow to +inf tie: the lowest wins, not the largest logit')
    lg = -np.abs(normal()) - F32(0.1)
    lg[n_lig - 1], lg[far] = -0.0, 0.0
    row(arg, 'negative_zero', lg, n_lig - 1, '-0.0 == 0.0: the lowest wins')
    lg = -rng.uniform(0.1, 10.0, size=n).astype(F32)
    row(arg, 'negative', lg, ar_pick_ref(lg, 100.0)[0], 'all logits negative and finite')
    # ---- sampling at AR_SAMPLE_T ----
    us = [('u0', F32(0)), ('u_half', F32(0.5)), ('u_top', F32(1) - F32(2.0 ** -24))] + [(f'u_{k}_over_n', _fp32_below(k / n)) for k in (1, n_lig, n - 1)]
    for name, u in us:
        row(smp, f'zeros_{name}', np.zeros(n), int(np.floor(np.float64(u) * n)), 'p = 1 everywhere, the sums are exact integers: floor(u n)', u=u)
    m = n_lig + 2 * per + 1
    lg = (2 * normal()).astype(F32)
    lg[:m:2], lg[1:m:2] = np.nan, -np.inf
    row(smp, 'leading_zero_mass', lg, m, 'a leading run of NaN and -inf with u = 0: the first entry whose p > 0', u=0.0)
    for name, u in (('u1e-6', 1e-6), ('u_half', 0.5), ('u_top', F32(1) - F32(2.0 ** -24))):
        lg = (2 * normal()).astype(F32)
        lg[far] = np.inf
        row(smp, f'one_inf_{name}', lg, far, 'one +inf logit holds all the mass that fp64 can see', u=u)
    for name, u, at in (('first', 0.25, n_lig - 1), ('second', 0.75, far)):
        lg = (2 * normal()).astype(F32)
        lg[n_lig - 1], lg[far] = 15.0, 20.0
        row(smp, f'two_overflows_{name}', lg, at, 'lg * 6 > 88.73 at two entries: both expf overflow and are clamped to FLT_MAX', u=u)
    row(smp, 'all_neg_inf', np.full(n, -np.inf), n - 1, 'a total of 0: the documented fall-through to n - 1', u=0.5)
    for i in range(AR_RANDOM_ROWS):
        lg, u = (2 * normal()).astype(F32), F32(rng.random(dtype=np.float32))
        row(smp, f'random{i}', lg, ar_pick_ref(lg, AR_SAMPLE_T, u)[0], 'against ar_pick_ref, margin >= AR_MARGIN', u=u)
    return dict(argmax=arg, sample=smp)


def chain_complex(n_lig, n_rec, seed=23):
    """a synthetic complex of exactly (n_lig, n_rec) nodes: synthetic.make_complex's receptor with a chain ligand in its pocket (make_ligand's smallest
    ligand has 18 atoms), built as adversarial_geometry.ligand builds its chains"""
    import adversarial_geometry as ag
    from disco_diffdock_amd import synthetic
    c = synthetic.make_complex(seed, n_res=n_rec, n_lig=20)
    rng = np.random.default_rng(seed + n_lig)
    pos = ag._chain_positions(n_lig, rng, planar=False)
    pos = pos - pos.mean(0) + c['lig_pos'].mean(0)
    bonds = [(i, i + 1) for i in range(n_lig - 1)]
    edge_mask, mask_rotate = synthetic.transformation_mask(n_lig, bonds)
    ei = np.zeros((2, 2 * len(bonds)), np.int64)
    for bi, (a, b) in enumerate(bonds):
        ei[:, 2 * bi], ei[:, 2 * bi + 1] = (a, b), (b, a)
    ea = np.zeros((2 * len(bonds), 4), np.float32)
    ea[:, 0] = 1
    c.update(lig_x=np.stack([rng.integers(0, d, size=n_lig) for d in synthetic.LIG_FEATURE_DIMS], 1), lig_pos=pos.astype(np.float32), bond_index=ei, bond_attr=ea,
             edge_mask=edge_mask, mask_rotate=mask_rotate)
    assert len(c['lig_pos']) == n_lig and len(c['rec_pos']) == n_rec
    return c


# ------------------------------------------------------------------------------------------------------------------------------------
# the AR predictors
# ------------------------------------------------------------------------------------------------------------------------------------
AR_LOGITS_CASES = ((128, 24, False, 'hard'), (96, 16, False, 'hard'), (40, 4, True, None))      # (H, ns, latent_no_batchnorm, BatchNorm statistics)
AR_LOGITS_COMPLEX = dict(seed=23, n_lig=11, n_rec=43, B=3)      # 33 ligand rows: one tile of 32 plus one row; 129 residue rows: four tiles plus one row
PREDICTORS = ('latent_s_predictor', 'latent_r_predictor')


def ar_state_dict(cfg, H, ns, no_bn, bn_stats, seed=31):
    """oracle.ar_ref.random_ar_state_dict at hidden width H and ns, then: no_bn drops every BatchNorm key; bn_stats == 'hard' overwrites the statistics -
    running_var a mix of 1e-6, 1e-5 and 1 (the fold's eps decides the scale of two thirds of the units), weight with a quarter of its entries negative and one
    exactly 0, running_mean = 3 * randn.  -> (state dict, claims)"""
    import torch
    from oracle import ar_ref
    P = ar_ref.random_ar_state_dict(cfg, ar_ns=ns, hidden=H, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    claims = dict(H=H, ns=ns, no_bn=no_bn)
    for name in PREDICTORS:
        for i in (1, 5):
            pre = f'{name}.{i}.'
            if no_bn:
                for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'):
                    del P[pre + k]
            elif bn_stats == 'hard':
                P[pre + 'running_var'] = torch.tensor([1e-6, 1e-5, 1.0])[torch.randint(0, 3, (H,), generator=g)]
                w = P[pre + 'weight'].clone()
                perm = torch.randperm(H, generator=g)
                w[perm[:H // 4]] *= -1
                w[perm[H // 4]] = 0.0
                P[pre + 'weight'] = w
                P[pre + 'running_mean'] = 3 * torch.randn(H, generator=g)
            elif bn_stats is not None:
                raise ValueError(bn_stats)
    return P, claims


def ar_mlp_ref(x_rows, P, prefix, ns, dtype=np.float64):
    """One predictor on node rows [N, W] -> [N] in ``dtype``: [x[:, :ns] | x[:, -ns:]] -> Linear -> BatchNorm1d(eval, eps 1e-5; none where the keys are absent)
    -> ReLU -> Linear -> BatchNorm -> ReLU -> Linear, from the checkpoint tensors UNFOLDED (the device folds the BatchNorms into the Linears)."""
    c = lambda k: np.asarray(P[f'{prefix}.{k}'].detach().cpu().numpy(), np.float64).astype(dtype)
    x = np.asarray(x_rows, np.float64).astype(dtype)
    h = np.concatenate([x[:, :ns], x[:, x.shape[1] - ns:]], 1)
    for lin, bn in ((0, 1), (4, 5)):
        h = h @ c(f'{lin}.weight').T + c(f'{lin}.bias')
        if f'{prefix}.{bn}.running_var' in P:
            h = (h - c(f'{bn}.running_mean')) / np.sqrt(c(f'{bn}.running_var') + dtype(1e-5)) * c(f'{bn}.weight') + c(f'{bn}.bias')
        h = np.maximum(h, dtype(0))
    out = h @ c('8.weight').T + c('8.bias')
    assert out.dtype == dtype
    return out[:, 0]


def ar_logits_ref(lig_rows, rec_rows, P, ns, B, dtype=np.float64):
    """[B, n_lig + n_rec]: graph b's ligand atoms, then its residues (pretrained_score_encoder.py:84-88), from the two tables of node rows [B * n, W]"""
    sl, sr = ar_mlp_ref(lig_rows, P, PREDICTORS[0], ns, dtype), ar_mlp_ref(rec_rows, P, PREDICTORS[1], ns, dtype)
    n_l, n_r = len(sl) // B, len(sr) // B
    return np.stack([np.concatenate([sl[b * n_l:(b + 1) * n_l], sr[b * n_r:(b + 1) * n_r]]) for b in range(B)])
