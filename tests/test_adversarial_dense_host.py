"""CPU tests of tests/adversarial_dense.py: the helper behind tests/test_gpu_dense_adversarial.py is itself held to account here, without a GPU.

* fma32 is a correctly rounded fp32 fused multiply-add: the constructed double-rounding case, and random and near-tie triples against fractions.Fraction
* its forms in fp64 are the project's closed forms (radial_hidden_ref, edge_embedding_ref, latent_embedding_ref, head_conv_ref) on plain operands
* S is tight: on non-negative operands the ABS form is the fp64 value
* every generator's claims hold (the generators assert them; the claims about outputs are asserted here); the eemb cases have no ambiguous ReLU branch
* an fp32 numpy evaluation of every op in two summation orders, and for rhid the emulator written from the kernels' headers, stays under the bar on every class,
  table, graph and shape the GPU test uses; the largest err / (u S) per op and output is printed (and kept in the helper's docstring)
* teeth: named mutants of that evaluation exceed the bar on the class built for them; the rel_err of the block the older tests judge is printed beside each"""
from fractions import Fraction

import numpy as np
import pytest

import adversarial_dense as ad
import edge_embedding_ref as eer
import head_conv_ref as hcr
import latent_embedding_ref as lar
import radial_hidden_ref as rhr
from adversarial_dense import ABS, FP32_ORDERS, FP64, U
from helpers import rel_err

F32 = np.float32
FIGURES = {}      # op.output -> the largest err / (u S) (eemb's row readers: err / bar) of the reference evaluations
REDRAWS = {}


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return a.size == 0 or np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


def _figure(key, got, ref, S, n=None):
    on = S > 0
    if on.any():
        scale = U * S if n is None else ad.bar(n, S)
        FIGURES[key] = max(FIGURES.get(key, 0.0), float((np.abs(np.asarray(got, np.float64) - ref)[on] / np.broadcast_to(scale, S.shape)[on]).max()))


def _ratio(got, M, k):
    return ad.worst(got, M[k][0], M[k][2], M[k][1])


# ---- 1. fma32 ----------------------------------------------------------------------------------------------------------------------------------
def _round_f32(x):
    """a Fraction rounded to the nearest fp32 number, ties to even"""
    if x == 0:
        return F32(0)
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    return F32(sign * float(round(x / q) * q))      # (round(Fraction): half to even; the product is an fp32 number, exact as a float)


def test_fma32_on_the_constructed_case():
    a, b, c = F32(2.0 ** -24 * (1 + 2.0 ** -20)), F32(1 - 2.0 ** -20), F32(1 + 2.0 ** -23)
    assert float(a) == 2.0 ** -24 * (1 + 2.0 ** -20) and float(b) == 1 - 2.0 ** -20
    assert float(F32(np.float64(a) * np.float64(b) + np.float64(c))) == 1 + 2.0 ** -22      # the plain form rounds twice
    assert float(ad.fma32(a, b, c)) == 1 + 2.0 ** -23
    assert ad.fma32(np.ones((3, 1), F32), np.ones((1, 4), F32), F32(1)).shape == (3, 4) and ad.fma32(F32(2), F32(3), F32(4)).shape == ()


def test_fma32_against_exact_rational_arithmetic():
    rng = np.random.default_rng(1)
    n = 1500
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3])).astype(F32)      # cancelling: the sum is the product's low half
    # near ties: c = +-m in [1, 2) and a * b = +-2^-24 (1 - i^2 2^-46), half an ulp of m less a sliver that the fp64 sum cannot hold: the sum sits a hair
    # off the midpoint of two fp32 numbers, on either side of it by the signs
    m = (1 + rng.integers(0, 2 ** 23, n) * 2.0 ** -23).astype(F32) * rng.choice([-1, 1], n).astype(F32)
    i = rng.integers(1, 200, n)
    a2 = (2.0 ** -24 * (1 + i * 2.0 ** -23)).astype(F32) * rng.choice([-1, 1], n).astype(F32)
    b2 = (1 - i * 2.0 ** -23).astype(F32)
    assert np.array_equal(np.abs(a2.astype(np.float64)) * b2, 2.0 ** -24 * (1 - (i * 2.0 ** -23) ** 2))
    A, B, C = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, m])
    got = ad.fma32(A, B, C)
    plain = (A.astype(np.float64) * B + C).astype(F32)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(A, B, C)], F32)
    assert np.array_equal(got.view(np.int32)[want != 0], want.view(np.int32)[want != 0]) and not got[want == 0].any()
    print(f'fma32: {len(A)} triples against exact rationals; the plain fp64 form differs from the true fma on {int((plain != want).sum())} of them')
    assert (plain != want).any()      # the triples do reach the double rounding


def test_every_shape_used_has_slices_of_512():
    sizes = [len(ad.rhid_layout(n)['src']) for n in ad.RHID_LAYOUTS] + [len(ad.graph(n)['src']) for n in ad.GRAPHS] + list(ad.EEMB_E)
    assert all(ad.slice_len(E) == ad.SLICE for E in sizes) and max(sizes) == 513 and ad.slice_len(240 * 512 + 1) == 576


# ---- 2. the forms ------------------------------------------------------------------------------------------------------------------------------
def test_rhid_fp64_forms_are_the_closed_forms():
    lay = ad.rhid_layout('degrees')
    rng = np.random.default_rng(2)
    f = lambda *s: rng.standard_normal(s).astype(F32)
    E, N, G = len(lay['src']), lay['N'], len(lay['offsets']) - 1
    o = dict(xs=f(N, 24), emb=f(E, 24), w1=f(G, 72, 72), b1=f(G, 72), g=f(E, 72))
    for p in ad.RHID_P:
        keep, s = rhr.keep_mask(77, E, p), rhr.scale(p)
        want_h = rhr.forward(o['xs'], lay['src'], lay['dst'], o['emb'], lay['offsets'], o['w1'], o['b1'], keep, s)
        got = ad.rhid_evaluate(FP64, lay, o, keep, s, want_h != 0)
        want = rhr.backward(o['xs'], lay['src'], lay['dst'], o['emb'], lay['offsets'], o['w1'], want_h != 0, s, o['g'])
        assert _close(got['h'], want_h) and all(_close(got[k], v) for k, v in zip(('grad_xs', 'grad_emb', 'grad_w1', 'grad_b1'), want))


@pytest.mark.parametrize('head', (0, 1))
def test_hconv_fp64_forms_are_the_closed_forms(head):
    gr = ad.graph('degrees')
    rng = np.random.default_rng(3)
    f = lambda *s: rng.standard_normal(s).astype(F32)
    E, K, W = len(gr['src']), hcr.K[head], hcr.W[head]
    o = dict(x=f(gr['n_in'], 84), sh=f(E, 4), h=f(E, K), w2=f(W, K), b2=f(W), g=f(gr['n_out'], hcr.DOUT[head]))
    got = ad.hconv_evaluate(FP64, head, gr, o)
    args = (head, o['x'], o['sh'], o['h'], o['w2'], o['b2'], gr['src'], gr['dst'], gr['n_out'])
    assert _close(got['out'], hcr.forward(*args))
    assert all(_close(got[k], v) for k, v in zip(('grad_x', 'grad_h', 'grad_w2', 'grad_b2'), hcr.vjp(*args, o['g'])))


@pytest.mark.parametrize('cfg', list(ad.EEMB_CONFIGS))
def test_eemb_fp64_forms_are_the_closed_forms(cfg):
    c = ad.EEMB_CONFIGS[cfg]
    for p in (0.0, 0.25):
        o = ad.eemb_operands('sig_spread', cfg, 130)
        keep, s, on = ad.eemb_pattern(cfg, o, p, 5)
        got = ad.eemb_evaluate(FP64, cfg, o, keep, s, on)
        oo = dict(o, zero_latent=c['zero'], unc_a=o.get('unc_a') if c['unc'] else None)
        if c['L']:
            assert _close(got['emb'], lar.forward(oo, o, c['L'], keep, s))
            want = lar.backward(oo, dict(o, uemb=o.get('uemb')), c['L'], o['g'], keep, s)
            assert all(_close(got[k], want[k]) for k in lar.NAMES)
        else:
            emb, sh, _ = eer.forward(oo, o['w1'], o['b1'], o['w2'], o['b2'], keep, s)
            assert _close(got['emb'], emb) and _close(got['sh'], sh)
            assert all(_close(got[k], v) for k, v in zip(('grad_w1', 'grad_b1', 'grad_w2', 'grad_b2'), eer.backward(oo, o['w1'], o['b1'], o['w2'], o['g'], keep, s)))


# ---- 3. S --------------------------------------------------------------------------------------------------------------------------------------
def test_S_is_tight_on_nonnegative_operands():
    absd = lambda o, keys: {k: (np.abs(v) if k in keys else v) for k, v in o.items()}
    lay = ad.rhid_layout('table0')
    o = absd(ad.rhid_operands('unit_spread', 'table0'), ('xs', 'emb', 'w1', 'b1', 'g'))
    E = len(lay['src'])
    keep = rhr.keep_mask(3, E, 0.25)
    for k, (ref, S, n) in ad.rhid_measures(lay, o, 0.25, 3, keep).items():
        assert (ref >= 0).all() and _close(S, ref), k
    gr = ad.graph('degrees')
    for head in (0, 1):
        o = absd(ad.hconv_operands('column_spread', head, 'degrees'), ('x', 'sh', 'h', 'w2', 'b2', 'g'))
        if head == 0:
            o['x'][:, 24:60] = 0      # no cross rows: there S is tight
        for k, (ref, S, n) in ad.hconv_measures(head, gr, o).items():
            if head == 0 and k == 'grad_x':      # (the vector columns of grad_x still hold the adjoint's cross products)
                ref, S = np.delete(ref, np.s_[24:60], 1), np.delete(S, np.s_[24:60], 1)
            assert (ref >= 0).all() and _close(S, ref), (head, k)
    o = absd(ad.eemb_operands('out_spread', 'lat2', 65), ('w1', 'b1', 'w2', 'b2', 'g', 'sig', 'lat_a', 'lat_b', 'uemb'))
    keep, s, on = ad.eemb_pattern('lat2', o, 0.25, 3)
    assert np.array_equal(on, keep)
    ref, S = ad.eemb_evaluate(FP64, 'lat2', o, keep, s, on), ad.eemb_evaluate(ABS, 'lat2', o, keep, s, on)
    for k in ref:
        assert _close(S[k], np.abs(ref[k])) and (k == 'sh' or (ref[k] >= 0).all()), k


# ---- 4. the classes: claims, S >= |ref|, the fp32 evaluations and the emulator under the bar -----------------------------------------------------------
@pytest.mark.parametrize('layout', ad.RHID_LAYOUTS)
@pytest.mark.parametrize('cls', ad.RHID_CLASSES)
def test_rhid_classes(cls, layout):
    lay, o = ad.rhid_layout(layout), ad.rhid_operands(cls, layout)
    E = len(lay['src'])
    for p in ad.RHID_P:
        emu = ad.rhid_emulate(lay, o, p, ad.RHID_SEED)
        pattern = emu['h'] != 0
        M = ad.rhid_measures(lay, o, p, ad.RHID_SEED, pattern)
        keep, s = rhr.keep_mask(ad.RHID_SEED, E, p), rhr.scale(p)
        assert not pattern[~keep].any() and (p == 0 or 0.15 < (~keep).mean() < 0.35)
        evs = [('emulator', emu)] + [(f'fp32.{i}', ad.rhid_evaluate(m, lay, o, keep, s, pattern)) for i, m in enumerate(FP32_ORDERS)]
        for tag, ev in evs:
            for k, (ref, S, n) in M.items():
                assert ev[k].dtype == F32 and np.all(S >= np.abs(ref) * (1 - 1e-12))
                ratio, where = ad.worst(ev[k], ref, n, S)
                assert ratio <= 1, (tag, p, ad.rhid_locate(k, where, lay), ratio)
                _figure(f'rhid.{"emulator" if tag == "emulator" else "fp32"}.{k}', ev[k], ref, S)
        cl = o['claims']
        if cls == 'dead':
            zg = cl['zero_group']
            if zg is not None:
                sl = slice(lay['offsets'][zg], lay['offsets'][zg + 1])
                assert not M['grad_w1'][1][zg].any() and not M['grad_b1'][1][zg].any() and not M['grad_emb'][1][sl].any() and not M['h'][0][sl].any()
                assert not emu['grad_w1'][zg].any() and not emu['grad_emb'][sl].any() and not emu['h'][sl].any()
            assert M['grad_w1'][0].any() and (pattern[cl['lone_edges']].sum(1) <= 1).all()
        empty = np.nonzero(np.diff(lay['offsets']) == 0)[0]
        for g in empty:
            assert not M['grad_w1'][1][g].any() and not M['grad_b1'][1][g].any()
        deg = np.bincount(lay['src'], minlength=lay['N']) + np.bincount(lay['dst'], minlength=lay['N'])
        assert not M['grad_xs'][1][deg == 0].any()


@pytest.mark.parametrize('gname', ad.GRAPHS)
@pytest.mark.parametrize('head', (0, 1))
@pytest.mark.parametrize('cls', ad.HCONV_CLASSES)
def test_hconv_classes(cls, head, gname):
    gr = ad.graph(gname)
    for variant in (('x', 'g') if cls == 'zero_blocks' else ('x',)):
        o = ad.hconv_operands(cls, head, gname, variant=variant)
        M = ad.hconv_measures(head, gr, o)
        for i, m in enumerate(FP32_ORDERS):
            ev = ad.hconv_evaluate(m, head, gr, o)
            for k, (ref, S, n) in M.items():
                assert ev[k].dtype == F32 and np.all(S >= np.abs(ref) * (1 - 1e-12))
                ratio, where = ad.worst(ev[k], ref, n, S)
                assert ratio <= 1, (i, ad.hconv_locate(k, where, head, gr), ratio)
                _figure(f'hconv.{("centre", "torsion")[head]}.{k}', ev[k], ref, S)
        ds, dd = np.bincount(gr['src'], minlength=gr['n_out']), np.bincount(gr['dst'], minlength=gr['n_in'])
        assert not M['out'][1][ds == 0].any() and not M['grad_x'][1][dd == 0].any()      # a node without edges: S = 0
        if head == 1:
            assert not M['grad_x'][1][:, :24].any() and not M['grad_x'][1][:, 60:].any()      # the torsion head reads neither a nor c
        if cls == 'zero_blocks':
            z = o['claims']['zero_slots']
            assert not M['grad_w2'][1][z].any() and not M['grad_b2'][1][z].any() and M['grad_w2'][0].any()
        if cls == 'relu_sparse':
            assert not o['h'][o['claims']['dead_edges']].any()


@pytest.mark.parametrize('cfg', list(ad.EEMB_CONFIGS))
@pytest.mark.parametrize('cls', ad.EEMB_CLASSES)
def test_eemb_classes(cls, cfg):
    c = ad.EEMB_CONFIGS[cfg]
    for case in ad.eemb_cases():
        if case[:2] != (cls, cfg):
            continue
        E = case[2]
        o, p = ad.eemb_operands(cls, cfg, E), ad.eemb_p(cls, E)
        REDRAWS[f'{cls}.{cfg}.E{E}'] = o['redraws']
        assert not ad.eemb_kinks(cfg, o).any()      # the cap of ambiguous ReLU branches is 0
        keep, s, on = ad.eemb_pattern(cfg, o, p, ad.EEMB_SEED)
        M = ad.eemb_measures(cfg, o, p, ad.EEMB_SEED)
        for i, m in enumerate(FP32_ORDERS):
            ev = ad.eemb_evaluate(m, cfg, o, keep, s, on)
            pre32 = ad.ee_row(m, cfg, o) @ o['w1'].T + o['b1']
            assert np.array_equal(keep & (pre32 > 0), on)      # no branch is ambiguous: the fp32 evaluation takes the fp64 pattern
            for k, (ref, S, n) in M.items():
                assert ev[k].dtype == F32
                ratio, where = ad.worst(ev[k], ref, n, S)
                assert ratio <= 1, (i, E, ad.eemb_locate(k, where, cfg), ratio)
                _figure(f'eemb.{k.replace("_a", "").replace("_b", "") if "lat" in k else k}', ev[k], ref, np.broadcast_to(S, ref.shape),
                        n if k in ('emb', 'grad_w1', 'grad_w2') else None)
        if cls == 'lengths':
            assert np.array_equal(M['sh'][0][0], [1, 0, 0, 0])
            assert np.array_equal(ad.eemb_evaluate(FP32_ORDERS[0], cfg, o, keep, s, on)['sh'][0], np.array([1, 0, 0, 0], F32))
        if c['zero']:
            assert not M['grad_lat_a'][1].any() and not M['grad_lat_b'][1].any() and not M['grad_w1'][1][:, c['F'] + 64:].any()
        if c['L'] and not c['unc']:
            assert not M['grad_uemb'][1].any()


# ---- 5. teeth ----------------------------------------------------------------------------------------------------------------------------------
def test_rhid_mutants_exceed_the_bar():
    fp32, p, seed = FP32_ORDERS[0], 0.25, ad.RHID_SEED
    out = []

    def case(cls, layout):
        lay, o = ad.rhid_layout(layout), ad.rhid_operands(cls, layout)
        emu = ad.rhid_emulate(lay, o, p, seed, parts=True)
        keep, s = rhr.keep_mask(seed, len(lay['src']), p), rhr.scale(p)
        return lay, o, emu, keep, s, ad.rhid_measures(lay, o, p, seed, emu['h'] != 0)

    # the smallest unit's bias dropped
    lay, o, emu, keep, s, M = case('unit_spread', 'table0')
    cu = o['claims']['small_unit']
    b1 = o['b1'].copy()
    b1[:, cu] = 0
    h = ad.rhid_evaluate(fp32, lay, dict(o, b1=b1), keep, s, emu['h'] != 0)['h']
    r, where = _ratio(h, M, 'h')
    old = rel_err(h, M['h'][0])
    assert r > 1 and where[1] == cu and old < 1e-5      # the block bar of the older tests lets it through: the gap
    out.append(f'the smallest unit\'s bias dropped (unit_spread, h) {r:.1e} (rel_err of h {old:.1e}: a pass at 1e-5)')
    # w1 rounded to fp16
    lay, o, emu, keep, s, M = case('column_spread', 'table0')
    with np.errstate(under='ignore'):
        w16 = o['w1'].astype(np.float16).astype(F32)
    h = ad.rhid_evaluate(fp32, lay, dict(o, w1=w16), keep, s, emu['h'] != 0)['h']
    r = _ratio(h, M, 'h')[0]
    assert r > 1
    out.append(f'w1 rounded to fp16 (column_spread, h) {r:.1e} (rel_err of h {rel_err(h, M["h"][0]):.1e})')
    # one edge, a slice's last, left out of the slice's grad_w1
    lay, o, emu, keep, s, M = case('edge_spread', 'table1')
    e = int(o['claims']['last_edges'][0])
    assert e == 511 and emu['gpre'][e].any()
    g = o['g'].copy()
    g[e] = 0
    gw1 = ad.rhid_evaluate(fp32, lay, dict(o, g=g), keep, s, emu['h'] != 0)['grad_w1']
    r = _ratio(gw1, M, 'grad_w1')[0]
    assert r > 1
    out.append(f'one edge left out of a slice\'s grad_w1 (edge_spread) {r:.1e} (rel_err of grad_w1 {rel_err(gw1, M["grad_w1"][0]):.1e})')
    # the dst sum of one node left out
    lay, o, emu, keep, s, M = case('unit_spread', 'degrees')
    node = 10      # twenty edges as dst, none as src
    assert (lay['dst'] == node).sum() == 20
    rows_dst = emu['gin'][:, 48:].copy()
    assert _ratio((ad.seg_ref(emu['gin'][:, 24:48], lay['src'], lay['N']) + ad.seg_ref(rows_dst, lay['dst'], lay['N'])).astype(F32), M, 'grad_xs')[0] <= 1
    rows_dst[lay['dst'] == node] = 0
    gxs = (ad.seg_ref(emu['gin'][:, 24:48], lay['src'], lay['N']) + ad.seg_ref(rows_dst, lay['dst'], lay['N'])).astype(F32)
    r, where = _ratio(gxs, M, 'grad_xs')
    assert r > 1 and where[0] == node
    out.append(f'the dst sum of one node left out (unit_spread, degrees, grad_xs) {r:.1e} (rel_err of grad_xs {rel_err(gxs, M["grad_xs"][0]):.1e})')
    print('rhid mutants, err / bar:\n    ' + '\n    '.join(out))


def test_hconv_mutants_exceed_the_bar():
    fp32, out = FP32_ORDERS[0], []
    gr = ad.graph('degrees')
    # S72 in place of S6 on block B; the cross product's sign in block C (the centre head)
    o = ad.hconv_operands('column_spread', 0, 'degrees')
    M = ad.hconv_measures(0, gr, o)
    assert _ratio(ad.hconv_evaluate(fp32, 0, gr, o)['out'], M, 'out')[0] <= 1
    for text, consts, cols in (('S72 in place of S6 on block B', {'B': hcr.S72}, slice(0, 6)), ('the cross product\'s sign in block C', {'C': -hcr.S72}, slice(6, 12))):
        got = ad.hconv_evaluate(fp32, 0, gr, o, consts)['out']
        r, where = _ratio(got, M, 'out')
        assert r > 1 and cols.start <= where[1] < cols.stop
        out.append(f'{text} (column_spread, out) {r:.1e} (rel_err of its block {rel_err(got[:, cols], M["out"][0][:, cols]):.1e})')
    # a dropped slot in the smallest channel (the torsion head): the one the older bar lets through
    o = ad.hconv_operands('column_spread', 1, 'degrees')
    M = ad.hconv_measures(1, gr, o)
    ch = o['claims']['small_channel']
    blk, row, col, chan, _, _ = ad.hc_slot_table(1)
    p = int(np.nonzero((chan == ch) & (row == 3))[0][0])
    w2, b2 = o['w2'].copy(), o['b2'].copy()
    w2[p], b2[p] = 0, 0
    got = ad.hconv_evaluate(fp32, 1, gr, dict(o, w2=w2, b2=b2))['out']
    r, where = _ratio(got, M, 'out')
    block = slice(0, 24) if ch < 24 else slice(24, 48)
    old = rel_err(got[:, block], M['out'][0][:, block])
    assert r > 1 and where[1] == ch and old < 1e-5
    out.append(f'a dropped slot in the smallest channel (column_spread, torsion, out) {r:.1e} (rel_err of its block {old:.1e}: a pass at 1e-5)')
    # a receiver's last row left out of its mean
    for head in (0, 1):
        o = ad.hconv_operands('channel_spread', head, 'degrees')
        M = ad.hconv_measures(head, gr, o)
        x, sh = o['x'][gr['dst']], o['sh']
        rows = ad.hc_rows(fp32, head, ad.hc_u(fp32, head, x, sh), ad.hc_weights(fp32, o))
        assert _ratio(ad.seg_ref(rows, gr['src'], gr['n_out'], mean=True), M, 'out')[0] <= 1
        rows[np.nonzero(gr['src'] == 0)[0][-1]] = 0      # the hub's last row
        got = ad.seg_ref(rows, gr['src'], gr['n_out'], mean=True)
        r, where = _ratio(got, M, 'out')
        assert r > 1 and where[0] == 0
        out.append(f'a receiver\'s last row left out of its mean (channel_spread, head {head}, out) {r:.1e} (rel_err of out {rel_err(got, M["out"][0]):.1e})')
    # one edge left out of grad_w2
    grn = ad.graph('one_node')
    for head in (0, 1):
        o = ad.hconv_operands('edge_spread', head, 'one_node')
        M = ad.hconv_measures(head, grn, o)
        e = int(o['claims']['last_edges'][0])
        assert e == 511 and o['h'][e].any()
        h = o['h'].copy()
        h[e] = 0
        got = ad.hconv_evaluate(fp32, head, grn, dict(o, h=h))['grad_w2']
        r = _ratio(got, M, 'grad_w2')[0]
        assert r > 1
        out.append(f'one edge left out of grad_w2 (edge_spread, head {head}) {r:.1e} (rel_err of grad_w2 {rel_err(got, M["grad_w2"][0]):.1e})')
    print('hconv mutants, err / bar:\n    ' + '\n    '.join(out))


def test_eemb_mutants_exceed_the_bar():
    fp32, out, seed = FP32_ORDERS[0], [], ad.EEMB_SEED

    def case(cls, cfg, E=130):
        o, p = ad.eemb_operands(cls, cfg, E), ad.eemb_p(cls, E)
        keep, s, on = ad.eemb_pattern(cfg, o, p, seed)
        M = ad.eemb_measures(cfg, o, p, seed)
        assert _ratio(ad.eemb_evaluate(fp32, cfg, o, keep, s, on)['emb'], M, 'emb')[0] <= 1
        return o, keep, s, on, M

    for text, cls, cfg, mutate in (('the sigma row taken from idx_b', 'sig_spread', 'plain64', {'sig_from_b': True}),
                                   ('the latent columns of the two sides swapped', 'latent_spread', 'lat2', {'swap_latent': True}),
                                   ('the unc_a uemb term dropped', 'out_spread', 'lat2', {'drop_unc': True})):
        o, keep, s, on, M = case(cls, cfg)
        got = ad.eemb_evaluate(fp32, cfg, o, keep, s, on, mutate=mutate)['emb']
        r = _ratio(got, M, 'emb')[0]
        assert r > 1
        out.append(f'{text} ({cls}, {cfg}, emb) {r:.1e} (rel_err of emb {rel_err(got, M["emb"][0]):.1e})')
    # the same term dropped in the smallest output column alone: the one the older bar lets through
    o, keep, s, on, M = case('out_spread', 'lat2')
    c0 = o['claims']['small_column']
    uemb = o['uemb'].copy()
    uemb[c0] = 0
    got = ad.eemb_evaluate(fp32, 'lat2', dict(o, uemb=uemb), keep, s, on)['emb']
    r, where = _ratio(got, M, 'emb')
    old = rel_err(got, M['emb'][0])
    assert r > 1 and where[1] == c0 and old < 1e-5
    out.append(f'the unc_a uemb term dropped in the smallest column (out_spread, lat2, emb) {r:.1e} (rel_err of emb {old:.1e}: a pass at 1e-5)')
    # the offsets shifted by one ulp.  This one stays UNDER the bar, and is printed as such: an ulp of an offset is 2 u |offset|, no more than what the
    # roundings of d (3.5 u d) and of t = d - offset (u |t|) may already move a column by, so no bar that admits an fp32 evaluation can tell it
    o, keep, s, on, M = case('lengths', 'plain64', 513)
    off = eer.offsets(o['start'], o['stop'])
    shifted = np.nextafter(off, F32(np.inf)).astype(F32)
    got = ad.eemb_evaluate(fp32, 'plain64', o, keep, s, on, mutate={'offsets': shifted})
    r = max(_ratio(got[k], M, k)[0] for k in ('emb', 'grad_w1', 'grad_w2'))
    out.append(f'the offsets shifted by one ulp (lengths, plain64; emb, grad_w1, grad_w2) {r:.1e} (rel_err of emb {rel_err(got["emb"], M["emb"][0]):.1e})')
    print('eemb mutants, err / bar:\n    ' + '\n    '.join(out))


def test_zz_print_the_figures():
    """(last in the file: the figures the other tests gathered, as the helper's docstring keeps them)"""
    for k in sorted(FIGURES):
        print(f'{k}: {FIGURES[k]:.2f}')
    print('eemb re-draws of b1 per case (cases not listed: 0):', {k: v for k, v in REDRAWS.items() if v})
