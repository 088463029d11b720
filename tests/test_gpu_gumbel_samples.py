"""ddk_gumbel_pick_samples (csrc/k_gumbel.hip): the one-hot latents of B samples of one complex from ONE table of logits.  Its contract is bitwise:
sample b's rows are ddk_gumbel_softmax_batch's ``out`` for the one graph with sample = sample0 + b; ``choices`` is the position of that op's maximum of
y.  The picks are also held against a host fp64 restatement (tests/oracle_latents_ref.py) wherever the top two are further apart than 1e-6, which the
host test (tests/test_oracle_sampling_host.py) shows to be everywhere for the seeds used here."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_latents_ref as olr
from helpers import _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


def _stream():
    from disco_diffdock_amd.runtime import stream_id
    return stream_id(olr.STREAM_NAME)


def _tables(dev, n_lig, n_rec, D):
    logits = olr.case_logits(n_lig, n_rec, D)
    return logits, torch.from_numpy(logits[:n_lig].copy()).to(dev), torch.from_numpy(logits[n_lig:].copy()).to(dev)


def _per_sample(ctx, dev, l, r, T, sample, seed=olr.SEED, draw=olr.DRAW):
    """the existing ragged op on the one graph: (out_l, out_r, the lowest position of the maximum of its y)"""
    ptr = lambda n: torch.tensor([0, n], dtype=torch.int64, device=dev)
    out_l, out_r, y_l, y_r = ctx.gumbel_softmax(l, r, ptr(l.shape[0]), ptr(r.shape[0]), T, seed, [_stream()], sample=sample, draw=draw)
    y = torch.cat([y_l, y_r]).cpu().numpy()
    return out_l, out_r, np.argmax(y, axis=0)      # (numpy's argmax: the first of equals)


@pytest.mark.parametrize('D', olr.DIMS)
@pytest.mark.parametrize('n_lig,n_rec', olr.SHAPES)
def test_bitwise_the_ragged_op_per_sample(ctx, dev, n_lig, n_rec, D):
    logits, l, r = _tables(dev, n_lig, n_rec, D)
    n = n_lig + n_rec
    for B in olr.BATCHES:
        for sample0 in olr.SAMPLE0S:
            want, gaps = olr.host_picks(logits, olr.SEED, _stream(), sample0, B, draw=olr.DRAW)
            assert (gaps > olr.GAP).all()      # (no case is left out below)
            for T in olr.TEMPERATURES:
                lat_l, lat_r, choices = ctx.gumbel_pick_samples(l, r, B, T, olr.SEED, _stream(), sample0=sample0, draw=olr.DRAW)
                assert tuple(lat_l.shape) == (B * n_lig, D) and tuple(lat_r.shape) == (B * n_rec, D) and tuple(choices.shape) == (B, D)
                assert choices.dtype == torch.int32
                got = choices.cpu().numpy()
                for b in range(B):
                    out_l, out_r, where = _per_sample(ctx, dev, l, r, T, sample0 + b)
                    assert torch.equal(_bits(lat_l[b * n_lig:(b + 1) * n_lig]), _bits(out_l)), (B, sample0, T, b)
                    assert torch.equal(_bits(lat_r[b * n_rec:(b + 1) * n_rec]), _bits(out_r)), (B, sample0, T, b)
                    assert got[b].tolist() == where.tolist(), (B, sample0, T, b)
                assert (got == want).all(), (B, sample0, T)      # the fp64 restatement's argmax
                if n >= 2:
                    assert (got != n // 2).all()                   # the -inf row is never chosen
                one = torch.cat([lat_l.reshape(B, n_lig, D), lat_r.reshape(B, n_rec, D)], dim=1)      # exactly one node per (b, d), at choices
                assert torch.equal(one.round().sum(1), torch.ones(B, D, device=dev))
                assert torch.equal(one.round().argmax(1).int(), choices)


def test_split_invariance(ctx, dev):
    """rows 3..4 of (B = 5, sample0 = 0) are (B = 2, sample0 = 3): a sample's draw is keyed by its global index, not by its place in a call"""
    for n_lig, n_rec in ((7, 23), (300, 800)):
        _, l, r = _tables(dev, n_lig, n_rec, 4)
        for T in olr.TEMPERATURES:
            a = ctx.gumbel_pick_samples(l, r, 5, T, olr.SEED, _stream(), sample0=0, draw=olr.DRAW)
            b = ctx.gumbel_pick_samples(l, r, 2, T, olr.SEED, _stream(), sample0=3, draw=olr.DRAW)
            assert torch.equal(_bits(a[0][3 * n_lig:]), _bits(b[0])) and torch.equal(_bits(a[1][3 * n_rec:]), _bits(b[1]))
            assert torch.equal(a[2][3:], b[2])
            assert not torch.equal(a[2][:2], b[2]) or n_lig + n_rec < 8      # (other samples, other picks)
            c = ctx.gumbel_pick_samples(l, r, 5, T, olr.SEED + 1, _stream(), sample0=0, draw=olr.DRAW)
            d = ctx.gumbel_pick_samples(l, r, 5, T, olr.SEED, _stream(), sample0=0, draw=olr.DRAW + 1)
            assert not torch.equal(a[2], c[2]) and not torch.equal(a[2], d[2])


def test_many_samples_follow_the_softmax(ctx, dev):
    """B = 4096 samples of six classes: every device pick is the host's, and the host's histogram is softmax(logits)'s (chi-square, 5 d.o.f., p = 1e-4):
    a kernel that left sample0 + b out of the key would give 4096 equal picks and fail both"""
    want, gaps = olr.host_picks(olr.STAT_LOGITS[:, None], olr.STAT_SEED, _stream(), 0, olr.STAT_B)
    assert (gaps > olr.GAP).all()
    chi2 = olr.chi_square(want, olr.STAT_LOGITS)
    print(f'chi-square of {olr.STAT_B} picks over {olr.STAT_N} classes: {chi2:.2f}')
    assert chi2 < olr.STAT_CHI2
    l = torch.from_numpy(olr.STAT_LOGITS[:4, None].copy()).to(dev)
    r = torch.from_numpy(olr.STAT_LOGITS[4:, None].copy()).to(dev)
    for T in olr.TEMPERATURES:
        _, _, choices = ctx.gumbel_pick_samples(l, r, olr.STAT_B, T, olr.STAT_SEED, _stream())
        assert (choices.cpu().numpy() == want).all()


def test_nan_logits_pick_nothing(ctx, dev):
    """a column of NaN logits compares with nothing: choices is -1 (include/ddk.h) and the rows hold no one, as the ragged op's; the other column and
    sampling's bookkeeping, which refuses an index outside the graph, are not disturbed"""
    n_lig, n_rec = 7, 23
    logits, l, r = _tables(dev, n_lig, n_rec, 2)
    l, r = l.clone(), r.clone()
    l[:, 1], r[:, 1] = float('nan'), float('nan')
    lat_l, lat_r, choices = ctx.gumbel_pick_samples(l, r, 3, 1.0, olr.SEED, _stream(), sample0=0, draw=olr.DRAW)
    want, _ = olr.host_picks(logits, olr.SEED, _stream(), 0, 3, draw=olr.DRAW)
    got = choices.cpu().numpy()
    assert (got[:, 1] == -1).all() and (got[:, 0] == want[:, 0]).all()
    assert bool(torch.isnan(lat_l[:, 1]).all()) and bool(torch.isnan(lat_r[:, 1]).all())
    for b in range(3):
        out_l, out_r, _ = _per_sample(ctx, dev, l, r, 1.0, b)
        assert torch.equal(_bits(lat_l[b * n_lig:(b + 1) * n_lig, 0]), _bits(out_l[:, 0])) and bool(torch.isnan(out_l[:, 1]).all())
        assert torch.equal(_bits(lat_r[b * n_rec:(b + 1) * n_rec, 0]), _bits(out_r[:, 0])) and bool(torch.isnan(out_r[:, 1]).all())


def test_refusals_leave_the_outputs_untouched(ctx, dev):
    DDK_ERR_INVALID = -1      # include/ddk.h
    n_lig, n_rec, D, B = 7, 23, 2, 3
    _, l, r = _tables(dev, n_lig, n_rec, D)
    lat_l, lat_r = torch.full((B * n_lig, D), 7.0, device=dev), torch.full((B * n_rec, D), 7.0, device=dev)
    choices = torch.full((B, D), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(B=B, D=D, l=l, n_lig=n_lig, r=r, n_rec=n_rec, T=1.0, sample0=0, draw=0, lat_l=lat_l, lat_r=lat_r, choices=choices, h=None):
        return ctx.L.ddk_gumbel_pick_samples(ctx.h if h is None else h, B, D, p(l), n_lig, p(r), n_rec, T, C.c_uint64(1), C.c_uint64(2), sample0, draw,
                                             p(lat_l), p(lat_r), p(choices), None)

    bad = [dict(B=0), dict(B=65537), dict(D=0), dict(D=5), dict(T=0.0), dict(T=-1.0), dict(T=float('inf')), dict(T=float('nan')), dict(draw=-1),
           dict(draw=1 << 20), dict(sample0=-1), dict(sample0=(1 << 31) - 2), dict(n_lig=-1), dict(n_rec=-1), dict(n_lig=1 << 31), dict(n_lig=(1 << 30), n_rec=(1 << 30)),
           dict(l=None), dict(r=None), dict(lat_l=None), dict(lat_r=None)]
    for kw in bad:
        assert call(**kw) == DDK_ERR_INVALID, kw
    assert call(h=C.c_void_p(0)) != 0      # a null context
    torch.cuda.synchronize()
    assert bool((lat_l == 7.0).all()) and bool((lat_r == 7.0).all()) and bool((choices == -7).all())
    # the same call without a violation runs (choices may be null; a side without nodes may pass null pointers)
    assert call(choices=None) == 0 and call() == 0
    assert call(l=None, n_lig=0, lat_l=None) == 0 and call(n_lig=0, n_rec=0, l=None, r=None, lat_l=None, lat_r=None) == 0
    torch.cuda.synchronize()
    assert bool((choices >= 0).all()) and bool((choices < n_lig + n_rec).all())
    # the wrapper refuses before the library is reached
    with pytest.raises(RuntimeError, match='D in 1..4'):
        ctx.gumbel_pick_samples(torch.zeros(3, 5, device=dev), torch.zeros(2, 5, device=dev), 2, 1.0, 1, 2)
    with pytest.raises(RuntimeError, match='temperature'):
        ctx.gumbel_pick_samples(l, r, 2, 0.0, 1, 2)
    with pytest.raises(RuntimeError, match='samples'):
        ctx.gumbel_pick_samples(l, r, 0, 1.0, 1, 2)
    with pytest.raises(RuntimeError, match='device tensors only'):
        ctx.gumbel_pick_samples(l.cpu(), r.cpu(), 2, 1.0, 1, 2)
