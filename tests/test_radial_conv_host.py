"""CPU tests of the radial conv's host side: Context.conv_graph (the checked graph tables the kernels trust), e3nn's BatchNorm as
_BatchNormParams.forward against the formulas written independently in numpy (tests/radial_conv_ref.py) and against oracle/e3nn_lite.batch_norm_eval,
the three entry points declared, exported and bound, and the workspace as a function of its arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import radial_conv_ref as rcr
import tp_backward_ref as tpr
from oracle import e3nn_lite
from oracle import score_model_ref as smr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CFG = smr.ScoreModelConfig()


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


# ---- conv_graph ----------------------------------------------------------------------------------------------------------------------
def test_conv_graph_tables():
    from disco_diffdock_amd.runtime import Context, ConvGraph
    rng = np.random.default_rng(3)
    n_in, n_out, E = 9, 6, 40
    src, dst = rng.integers(0, n_out, E), rng.integers(0, n_in, E)
    src[src == 4] = 0      # output node 4 receives nothing
    dst[dst == 7] = 2      # input node 7 sends nothing
    g = Context.conv_graph(torch.from_numpy(src), torch.from_numpy(dst), n_in, n_out)
    assert isinstance(g, ConvGraph) and (g.E, g.n_in, g.n_out) == (E, n_in, n_out)
    assert g.src.dtype == g.dst.dtype == g.src_order.dtype == g.dst_order.dtype == torch.int32
    assert g.src_ptr.dtype == g.dst_ptr.dtype == torch.int64
    assert np.array_equal(g.src.numpy(), src) and np.array_equal(g.dst.numpy(), dst)
    for idx, order, ptr, count, n in ((src, g.src_order, g.src_ptr, g.src_count, n_out), (dst, g.dst_order, g.dst_ptr, g.dst_count, n_in)):
        order, ptr, count = order.numpy(), ptr.numpy(), count.numpy()
        assert np.array_equal(order, np.argsort(idx, kind='stable'))      # by node, ascending edge id within a node
        assert np.array_equal(count, np.bincount(idx, minlength=n)) and ptr.shape == (n + 1,)
        assert ptr[0] == 0 and np.array_equal(np.diff(ptr), count)
        for node in range(n):
            mine = order[ptr[node]:ptr[node + 1]]
            assert np.array_equal(mine, np.flatnonzero(idx == node))
    assert g.src_count[4] == 0 and g.dst_count[7] == 0
    # a list and a [2, E] edge_index row work alike
    ei = torch.from_numpy(np.stack([src, dst]))
    g2 = Context.conv_graph(ei[0], ei[1], n_in, n_out)
    assert torch.equal(g2.src_order, g.src_order) and torch.equal(g2.dst_ptr, g.dst_ptr)


def test_conv_graph_without_edges_and_refusals():
    from disco_diffdock_amd.runtime import Context
    g = Context.conv_graph(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), 3, 2)
    assert g.E == 0 and g.src_order.shape == (0,) and g.src_ptr.tolist() == [0, 0, 0] and g.dst_ptr.tolist() == [0, 0, 0, 0]
    ok = torch.tensor([0, 1, 1])
    for src, dst in (([0, 1, 2], ok), ([0, -1, 1], ok), (ok, [0, 3, 1]), (ok, [-1, 0, 0])):
        with pytest.raises(RuntimeError, match='conv_graph'):
            Context.conv_graph(torch.as_tensor(src), torch.as_tensor(dst), 3, 2)
    with pytest.raises(RuntimeError, match='conv_graph'):
        Context.conv_graph(ok, ok[:2], 3, 2)
    with pytest.raises(RuntimeError, match='conv_graph'):
        Context.conv_graph(ok.float(), ok, 3, 2)


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------------
def _bn(l, seed, n=13):
    from disco_diffdock_amd.tensor_layers import _BatchNormParams
    muls = tpr.shape(l)['O']
    bn = _BatchNormParams(CFG.conv_irreps(l)[1]).double()
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, generator=gen, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(bn.bias.shape, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen, dtype=torch.float64) + 0.5)
    x = torch.randn(n, tpr.shape(l)['dout'], generator=gen, dtype=torch.float64) * 2 + 0.7
    return bn, muls, x


@pytest.mark.parametrize('l', [0, 3])
def test_batch_norm_training_matches_the_formulas(l):
    bn, muls, x = _bn(l, 10 + l)
    w, b = bn.weight.detach().numpy().copy(), bn.bias.detach().numpy().copy()
    rm, rv = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    assert w.shape == (sum(muls),) and b.shape == rm.shape == (muls[0],)      # 0o channels carry neither mean nor bias
    bn.train()
    for step in range(2):      # after one and after two calls
        xs = x + step
        got = bn(xs).detach().numpy()
        want, rm, rv = rcr.batch_norm(xs.numpy(), muls, w, b, rm, rv, training=True)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-12
        assert np.abs(bn.running_mean.numpy() - rm).max() < 1e-13 and np.abs(bn.running_var.numpy() - rv).max() < 1e-13
    if muls[3]:      # the 0o block: scaled by its norm alone, so a sign flip of its input flips its output (no mean, no bias)
        sl = slice(muls[0] + 3 * muls[1] + 3 * muls[2], None)
        flipped = x.clone()
        flipped[:, sl] *= -1
        a, c = bn(x).detach(), bn(flipped).detach()
        assert torch.equal(a[:, sl], -c[:, sl]) and not torch.allclose(a[:, :muls[0]], -c[:, :muls[0]])


@pytest.mark.parametrize('l', [0, 3])
def test_batch_norm_eval_equals_the_oracle(l):
    bn, muls, x = _bn(l, 20 + l)
    bn.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    got = bn(x)
    want = e3nn_lite.batch_norm_eval(x, CFG.conv_irreps(l)[1], bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var)
    assert (got - want).abs().max().item() < 1e-12
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])      # evaluation leaves the buffers alone
    mine, _, _ = rcr.batch_norm(x.numpy(), muls, bn.weight.detach().numpy(), bn.bias.detach().numpy(), before[0].numpy(), before[1].numpy(), training=False)
    assert np.abs(got.detach().numpy() - mine).max() < 1e-12


@pytest.mark.parametrize('l', [0, 3])
def test_batch_norm_training_equals_eval_on_the_batch_statistics(l):
    bn, muls, x = _bn(l, 30 + l)
    bn.train()
    trained = bn(x).detach()
    w, b = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    _, mean, norm = rcr.batch_norm(x.numpy(), muls, w, b, np.zeros(muls[0]), np.zeros(sum(muls)), training=True, momentum=1.0)      # the batch statistics
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(mean))
        bn.running_var.copy_(torch.from_numpy(norm))
    bn.eval()
    assert (bn(x).detach() - trained).abs().max().item() < 1e-12


def test_batch_norm_gradcheck():
    bn, muls, x = _bn(3, 40, n=7)
    bn.train()
    x = x.requires_grad_(True)

    f = lambda x, w, b: torch.func.functional_call(bn, {'weight': w, 'bias': b}, (x,))      # (the training output does not read the running buffers)
    assert torch.autograd.gradcheck(f, (x, bn.weight.detach().clone().requires_grad_(True), bn.bias.detach().clone().requires_grad_(True)), eps=1e-6, atol=1e-6)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(built):
    from disco_diffdock_amd import _lib, tensor_layers
    from disco_diffdock_amd.runtime import Context
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    assert re.search(r'\bint\s+ddk_rconv_forward\s*\(', hdr) and re.search(r'\bint\s+ddk_rconv_backward\s*\(', hdr)
    assert re.search(r'\bint64_t\s+ddk_rconv_workspace\s*\(', hdr)
    cdll = ctypes.CDLL(built)
    for name in ('ddk_rconv_forward', 'ddk_rconv_backward', 'ddk_rconv_workspace'):
        assert name in _lib.SYMBOLS and hasattr(cdll, name), name
    L = _lib.lib()
    count = lambda name: len(re.search(r'\bint(?:64_t)?\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr).group(1).split(','))
    assert len(L.ddk_rconv_forward.argtypes) == count('ddk_rconv_forward') == 19
    assert len(L.ddk_rconv_backward.argtypes) == count('ddk_rconv_backward') == 26
    assert len(L.ddk_rconv_workspace.argtypes) == count('ddk_rconv_workspace') == 6 and L.ddk_rconv_workspace.restype is ctypes.c_int64
    assert L.ddk_rconv_forward.argtypes[15] is ctypes.c_int64 and L.ddk_rconv_backward.argtypes[18] is ctypes.c_int64      # E
    assert callable(tensor_layers.fused_radial_conv) and callable(Context.rconv_forward) and callable(Context.rconv_backward)


def test_workspace_is_a_function_of_its_arguments(built):
    from disco_diffdock_amd import _lib
    L = _lib.lib()
    ws, images = L.ddk_rconv_workspace, L.ddk_rtp_backward_workspace
    pad = lambda n: (n + 3) // 4 * 4
    for l in range(5):
        s = tpr.shape(l)
        for E, G, n_in, n_out in ((0, 1, 0, 0), (1, 1, 1, 1), (33, 4, 9, 4), (1300, 2, 5, 5), (50000, 4, 2000, 2000)):
            assert ws(l, E, G, n_in, n_out, 0) == 4 * pad(E * s['dout'])      # the tensor product's rows, nothing else
            assert ws(l, E, G, n_in, n_out, 1) == 4 * (pad(n_out * s['dout']) + pad(E * s['din'])) + images(l, E, G)
    # never an [E, W] tensor: at the size of the memory test the backward's workspace is a fraction of one
    assert ws(3, 50000, 4, 2000, 2000, 1) < 4 * 50000 * tpr.shape(3)['W'] // 4
    for bad in ((-1, 10, 4, 3, 3, 0), (5, 10, 4, 3, 3, 0), (3, -1, 4, 3, 3, 1), (3, 2 ** 31, 4, 3, 3, 1), (3, 10, 0, 3, 3, 0), (3, 10, 5, 3, 3, 0),
                (3, 10, 4, -1, 3, 1), (3, 10, 4, 3, -1, 1), (3, 10, 4, 2 ** 31, 3, 1), (3, 10, 4, 3, 2 ** 31, 0)):
        assert ws(*bad) == -1, bad


def test_host_only_context_refuses_the_launches(built):
    from disco_diffdock_amd.runtime import Context
    ctx = Context(device=-1)
    ctx.finalize()
    one = ctypes.c_void_p(16)      # never dereferenced: the refusal comes first
    offs = (ctypes.c_int64 * 2)(0, 4)
    rc = ctx.L.ddk_rconv_forward(ctx.h, 3, one, 2, 2, one, one, one, one, one, one, offs, 1, one, one, 4, one, one, None)
    assert rc == -3 and b'host-only' in ctx.L.ddk_last_error(ctx.h)
    rc = ctx.L.ddk_rconv_backward(ctx.h, 3, one, 2, 2, one, one, one, one, one, one, one, one, offs, 1, one, one, one, 4, one, one, one, one, one, one, None)
    assert rc == -3 and b'host-only' in ctx.L.ddk_last_error(ctx.h)
    with pytest.raises(RuntimeError, match='at least one gradient'):
        ctx.rconv_backward(3, None, None, None, None, [0, 0], None, None, None, need=(False,) * 5)


def test_the_layer_no_longer_refuses_training_outright():
    """in training the layer reaches the device path (and refuses CPU tensors there), instead of raising 'inference only'"""
    from disco_diffdock_amd.tensor_layers import TensorProductConvLayer
    i_irr, o_irr = CFG.conv_irreps(1)
    layer = TensorProductConvLayer(i_irr, '1x0e+1x1o', o_irr, 72, faster=True, edge_groups=4, hidden_features=72)
    layer.train()
    s = tpr.shape(1)
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match='GPU only'):
        layer(torch.zeros(2, s['din']), ei, [torch.zeros(2, 72), torch.zeros(0, 72), torch.zeros(0, 72), torch.zeros(0, 72)], torch.zeros(2, 4))
