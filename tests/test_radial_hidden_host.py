"""CPU tests of the radial hidden layer's host side: the fp64 restatement the kernels are measured against (tests/radial_hidden_ref.py) equals torch
autograd of the composition it replaces (cat + Linear + ReLU + a given mask), the mask layout of include/ddk.h restated with tests/philox_ref.py keeps
what a dropout of rate p keeps, and ddk_rhid_workspace states its ranges."""
import numpy as np
import pytest
import torch

import radial_hidden_ref as ref


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


def _case(seed, N, offsets):
    rng = np.random.default_rng(seed)
    E, G = offsets[-1], len(offsets) - 1
    f = lambda *shape: rng.standard_normal(shape)
    return dict(xs=f(N, 24), emb=f(E, 24), src=rng.integers(0, N, E), dst=rng.integers(0, N, E), w1=f(G, 72, 72) / np.sqrt(72.0), b1=f(G, 72), g=f(E, 72))


@pytest.mark.parametrize('p', [0.0, 0.25])
def test_restatement_equals_autograd_of_the_composition(p):
    N, offsets = 9, [0, 3, 3, 20, 41]
    o = _case(7, N, offsets)
    E = offsets[-1]
    keep = ref.keep_mask(1234, E, p)
    s = ref.scale(p)
    assert (p == 0 and s == 1.0 and keep.all()) or (p > 0 and abs(s - 1 / (1 - p)) < 1e-7 and not keep.all() and keep.any())
    t = {k: torch.tensor(o[k], dtype=torch.float64, requires_grad=True) for k in ('xs', 'emb', 'w1', 'b1')}
    src, dst = torch.from_numpy(o['src']), torch.from_numpy(o['dst'])
    row = torch.cat([t['emb'], t['xs'][src], t['xs'][dst]], -1)
    pre = torch.cat([torch.nn.functional.linear(row[offsets[g]:offsets[g + 1]], t['w1'][g], t['b1'][g]) for g in range(4)])
    h = torch.relu(pre) * torch.from_numpy(keep) * s
    h.backward(torch.from_numpy(o['g']))
    got_h = ref.forward(o['xs'], o['src'], o['dst'], o['emb'], offsets, o['w1'], o['b1'], keep, s)
    np.testing.assert_allclose(got_h, h.detach().numpy(), rtol=0, atol=1e-12)
    got = ref.backward(o['xs'], o['src'], o['dst'], o['emb'], offsets, o['w1'], got_h != 0, s, o['g'])
    for name, a in zip(('xs', 'emb', 'w1', 'b1'), got):
        np.testing.assert_allclose(a, t[name].grad.numpy(), rtol=0, atol=1e-11, err_msg=name)
    assert not got[2][1].any() and not got[3][1].any()      # the empty group


def test_margin_is_the_fp32_dot_product_bound():
    o = _case(3, 5, [0, 12])
    pre, margin = ref.pre_activation(o['xs'], o['src'], o['dst'], o['emb'], [0, 12], o['w1'], o['b1'])
    a = ref.rows(o['xs'], o['src'], o['dst'], o['emb'])
    e, c = 4, 17
    assert margin[e, c] == pytest.approx(72 * 2.0 ** -23 * (np.abs(o['w1'][0, c] * a[e]).sum() + abs(o['b1'][0, c])), rel=1e-12)
    # an fp32 evaluation in any order stays inside it
    f32 = (a.astype(np.float32) @ o['w1'][0].astype(np.float32).T + o['b1'][0].astype(np.float32)).astype(np.float64)
    pre32, _ = ref.pre_activation(o['xs'].astype(np.float32), o['src'], o['dst'], o['emb'].astype(np.float32), [0, 12], o['w1'].astype(np.float32),
                                  o['b1'].astype(np.float32))
    assert (np.abs(f32 - pre32) <= margin).all()


def test_mask_layout():
    E, p = 4096, 0.1
    keep = ref.keep_mask(20240607, E, p)
    n = keep.size
    assert keep.shape == (E, 72) and n == 72 * 4096
    sigma = np.sqrt(n * p * (1 - p))
    assert abs(int(keep.sum()) - n * (1 - p)) < 4 * sigma      # the keep rate of a dropout of rate p, within 4 sigma of the binomial
    assert ref.keep_mask(20240607, E, 0.0).all()      # p == 0 keeps everything
    # a pure function of (seed, edge id, column): a window of edges is the same window of the mask; another seed is another mask
    assert np.array_equal(ref.keep_mask(20240607, 50, p, e0=1000), keep[1000:1050])
    other = ref.keep_mask(20240608, E, p)
    assert 0.1 < float((other != keep).mean()) < 0.3      # two independent masks differ on 2 p (1 - p) = 18 % of the elements
    # the layout itself, for one element, written out: counter (e_lo, e_hi, c / 4, tag), word c % 4, kept iff (word >> 8) * 2^-24 >= p
    import philox_ref
    e, c, seed = (1 << 32) + 5, 30, (7 << 32) | 9
    words = philox_ref.philox4x32_10((5, 1, c // 4, 0x52484944), (9, 7))
    u = np.float32(int(words[c % 4]) >> 8) * np.float32(2.0 ** -24)
    assert bool(ref.keep_mask(seed, 1, p, e0=e)[0, c]) == bool(u >= np.float32(p))


def test_workspace_ranges(built):
    from disco_diffdock_amd import _lib
    ws = _lib.lib().ddk_rhid_workspace
    pad = lambda n: (n + 3) // 4 * 4
    # per-edge src rows, per-edge dst rows, the dst sum per node, E / slice length + G images of [72][73]
    assert ws(0, 1, 0) == 72 * 73 * 4
    assert ws(70, 4, 11) == (2 * pad(70 * 24) + pad(11 * 24) + 4 * 72 * 73) * 4
    assert ws(1300, 1, 40) == (2 * 1300 * 24 + 40 * 24 + (2 + 1) * 72 * 73) * 4      # slices of 512 edges
    assert ws(3, 2, 1) == (2 * 72 + 24 + 2 * 72 * 73) * 4
    big = ws((1 << 31) - 1, 4, (1 << 31) - 1)
    assert big > 0 and big < 1 << 40
    for bad in ((-1, 1, 1), (1 << 31, 1, 1), (1, 0, 1), (1, 5, 1), (1, 1, -1), (1, 1, 1 << 31)):
        assert ws(*bad) == -1, bad
