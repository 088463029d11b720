"""CPU tests of the sampler's counter-based generator as tests/philox_ref.py restates it (DDK_RNG_LAYOUT 1 of include/ddk.h): the known answers of
Philox4x32-10 and FNV-1a, the counter layout, the extremes of the word -> draw conversions, and the statistical checks of tests/test_gpu_rng.py run on the
restatement with the SAME seeds and counts, which shows that the reference alone stays inside every threshold the device is held to."""
import os
import re

import numpy as np
import pytest

import philox_ref as pr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def _hex(words):
    return ' '.join('%08x' % int(w) for w in np.asarray(words).reshape(-1))


@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(ctr, key, want):
    assert _hex(pr.philox4x32_10(ctr, key)) == want


def test_fnv1a_vectors_and_the_shim():
    assert pr.fnv1a64('') == 0xcbf29ce484222325 and pr.fnv1a64('a') == 0xaf63dc4c8601ec8c
    from disco_diffdock_amd.runtime import stream_id
    for name in ('', 'a', 'foobar', '6qqw', 'liganden-äö'):
        assert stream_id(name) == pr.fnv1a64(name)
    assert stream_id('a') == 0xaf63dc4c8601ec8c and stream_id('foobar') == 0x85944171f73967e8


def test_header_and_shim_state_the_layout():
    """the published constants: the header's define, the generator header's constants, the Python shim's purposes and limits"""
    from disco_diffdock_amd import runtime, _lib
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    assert re.search(r'#define DDK_RNG_LAYOUT 1\b', hdr) and runtime.RNG_LAYOUT == 1
    for text in ('5.768', 'signed zero', '0xD2511F53', '0xCD9E8D57', '0x9E3779B9', '0xBB67AE85'):
        assert text in hdr, text
    src = open(os.path.join(ROOT, 'disco_diffdock_amd', 'csrc', 'k_philox.h')).read()
    for c in (pr.M0, pr.M1, pr.W0, pr.W1):
        assert ('0x%08X' % c) in src
    assert runtime.RNG_PURPOSES == pr.PURPOSE and (runtime.RNG_MAX_STEPS, runtime.RNG_MAX_COLS) == (1 << 20, 1024)
    for name in ('ddk_rng_noise', 'ddk_rng_initial', 'ddk_rng_uniform'):
        assert name in _lib.SYMBOLS
        m = re.search(r'int %s\((.*?)\);' % name, hdr, re.S)
        assert m, name
    assert 'k_rng.hip' in __import__('disco_diffdock_amd.build', fromlist=['SOURCES']).SOURCES


def test_value_does_not_depend_on_the_cut():
    """row (step, sample) of the noise is the same bits whatever B, sample0, step0 and steps cut it out of"""
    seed, stream = 99, pr.fnv1a64('cut')
    whole = pr.noise(seed, stream, 0, 12, 0, 7, 9)
    for sample0, B, step0, steps in ((0, 12, 0, 7), (5, 3, 2, 4), (11, 1, 6, 1), (0, 1, 0, 1), (4, 8, 3, 2)):
        part = pr.noise(seed, stream, sample0, B, step0, steps, 9)
        assert np.array_equal(part, whole[step0:step0 + steps, sample0:sample0 + B])
    tor, rot, tr = pr.initial(seed, stream, 0, 12, 9, 3.0)
    t2, r2, x2 = pr.initial(seed, stream, 7, 4, 9, 3.0)
    assert np.array_equal(t2, tor[7:11]) and np.array_equal(r2, rot[7:11]) and np.array_equal(x2, tr[7:11])
    assert np.array_equal(pr.initial(seed, stream, 7, 4, 5, 3.0)[0], tor[7:11, :5])      # fewer torsions: a prefix
    assert np.array_equal(pr.uniform(seed, stream, 3, 5, 4), pr.uniform(seed, stream, 0, 12, 4)[3:8])


def test_every_counter_field_changes_the_block():
    base = dict(seed=0x1122334455667788, stream=0x99aabbccddeeff00, sample=17, purpose=0, step=5, blk=2)
    b0 = pr.block(**base)
    changed = dict(seed_lo=dict(seed=base['seed'] ^ 1), seed_hi=dict(seed=base['seed'] ^ (1 << 32)), stream_lo=dict(stream=base['stream'] ^ 1),
                   stream_hi=dict(stream=base['stream'] ^ (1 << 32)), sample=dict(sample=18), step=dict(step=6), purpose=dict(purpose=1), block=dict(blk=3))
    seen = {_hex(b0)}
    for name, kw in changed.items():
        b = pr.block(**dict(base, **kw))
        assert not np.array_equal(b, b0), name
        seen.add(_hex(b))
    assert len(seen) == len(changed) + 1
    # the fields do not overlap in counter word 3: the largest step and block of one purpose are not the next purpose's first
    assert not np.array_equal(pr.block(1, 2, 0, 0, (1 << 20) - 1, 255), pr.block(1, 2, 0, 1, 0, 0))
    with pytest.raises(AssertionError):
        pr.block(1, 2, 0, 0, 1 << 20, 0)
    with pytest.raises(AssertionError):
        pr.block(1, 2, 0, 0, 0, 256)


def test_word_extremes_give_finite_bounded_draws():
    """u1 = 2^-24 (the largest radius) and u1 = 1 (radius 0), u2 = 0 and the largest u2, the quarter turns: finite, |z| <= 5.769, no NaN, exact zeros"""
    lo, hi = 0x00000000, 0xFFFFFFFF
    quarter = [q << 30 for q in range(4)]
    words = np.array([[a, b, c, d] for a in (lo, hi, 0xFF, 0xFFFFFF00) for b in (lo, hi, *quarter) for c in (lo, hi) for d in (lo, hi, *quarter)], np.uint64)
    z = pr.normals64(words)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.769
    assert abs(np.abs(pr.normals64(np.array([[lo, lo, lo, lo]], np.uint64))).max() - pr.Z_MAX) < 1e-12 and abs(pr.Z_MAX - 5.768) < 1e-3
    z1 = pr.normals64(np.array([[hi, 0x12345678, hi, 0x9abcdef0]], np.uint64))      # u1 = 1: r = 0
    assert (z1 == 0).all()
    zq = pr.normals64(np.array([[lo, quarter[1], lo, quarter[3]]], np.uint64))[0]     # 2 u2 = 1/2 and 3/2: the cosine is an exact zero
    assert zq[0] == 0 and zq[2] == 0 and abs(zq[1] - pr.Z_MAX) < 1e-12 and abs(zq[3] + pr.Z_MAX) < 1e-12
    u = pr.uniform32(np.array([lo, hi, 0xFF, 0x100], np.uint64))
    assert u.dtype == np.float32 and u[0] == 0 and u[1] == np.float32(1 - 2.0 ** -24) and u[2] == 0 and u[3] == np.float32(2.0 ** -24)
    t = pr.torsion32(np.array([lo, hi, 1 << 31], np.uint64))
    assert t.dtype == np.float32 and t[0] == -np.float32(np.pi) and t[1] < np.float32(np.pi) and t[2] == 0
    assert np.array_equal(pr.rotation64(np.zeros((1, 4)))[0], np.eye(3))
    assert np.array_equal(pr.rotation64(np.full((1, 4), 2.0 ** -32))[0], np.eye(3))      # |q|^2 = 2^-62: below the threshold


def test_noise_layout_zero_steps_and_padding():
    nc = np.array([[1, 0, 0], [0, 0, 0], [0, 0.5, 0], [0, 0, 2]], np.float32)
    z = pr.noise(3, 4, 5, 3, 2, 4, 9, 6, nc)
    full = pr.noise(3, 4, 5, 3, 2, 4, 9)
    assert (z[1] == 0).all() and (z[:, :, 6:] == 0).all()
    assert np.array_equal(z[[0, 2, 3], :, :6], full[[0, 2, 3], :, :6]) and (full != 0).all()
    # column c is normal c % 4 of block c / 4
    blk = pr.normals64(pr.block(3, 4, 6, 0, 4, 2))
    assert full[2, 1, 8] == blk[0]


def test_statistics_of_the_restatement():
    """the thresholds of tests/test_gpu_rng.py::test_statistics on the same seed and counts: the reference alone is inside every one"""
    z = pr.noise(pr.STAT_SEED, pr.STAT_STREAM, 0, step0=0, **pr.STAT_NORMALS)
    n = z.size
    assert n == 1 << 20
    mean, var, ks = pr.normal_statistics(z)
    b_mean, b_var, b_ks = pr.normal_statistics_bounds(n)
    print(f'restatement: |mean| {mean:.3e} < {b_mean:.3e}, |var - 1| {var:.3e} < {b_var:.3e}, KS {ks:.3e} < {b_ks:.3e}')
    assert mean < b_mean and var < b_var and ks < b_ks
    assert np.abs(z).max() <= 5.769
    _, rot, _ = pr.initial(pr.STAT_SEED, pr.STAT_STREAM, 0, pr.STAT_ROTATIONS, 0)
    m = np.abs(rot.mean(axis=0))
    print(f'restatement: rotation mean matrix max {m.max():.3e} < {pr.rotation_mean_bound(pr.STAT_ROTATIONS):.3e}')
    assert (m < pr.rotation_mean_bound(pr.STAT_ROTATIONS)).all()
    assert np.abs(rot.transpose(0, 2, 1) @ rot - np.eye(3)).max() < 1e-14 and np.linalg.det(rot).min() > 0.999


def test_seeded_keywords_are_refused_together_with_noise():
    """sampling(noise=..., seed=...) is a ValueError before anything touches a device"""
    from disco_diffdock_amd.sampling import sampling
    with pytest.raises(ValueError, match='noise'):
        sampling([object()], None, 3, None, None, None, 'cpu', None, None, noise=[None], seed=1)
