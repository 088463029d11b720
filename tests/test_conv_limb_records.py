"""CPU test of the f16-limb weight records a host-only context packs (conv_pack.hip: pack_x3; layouts in csrc/ddk_internal.h): the default two-limb form's
9 360-B W2 records and 9 216-B W1 tiles decoded with the offsets the kernel uses, re-added against the fp32 fragments they were split from, and held against
the three-limb records of a conv_kernel = 3 context (same hi and mid bits at the same offsets, which stay 13 968 B)."""
import numpy as np
import pytest

from oracle import score_model_ref as smr

CFG = smr.ScoreModelConfig()
LIMB = 4 * 1024 + 512
REC2, BIAS2, DESC2 = 2 * LIMB + 128 + 16, 2 * LIMB, 2 * LIMB + 128          # W2X2_TILE_BYTES, W2X2_BIAS_OFF, W2X2_DESC_OFF
REC3, BIAS3, DESC3 = 3 * LIMB + 128 + 16, 3 * LIMB, 3 * LIMB + 128          # W2X_TILE_BYTES, W2X_BIAS_OFF, W2X_DESC_OFF


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


def _limb(rec, limb):
    """one limb of a record as fp64 [36 registers][64 lanes]: register r of a lane half = element r % 8 of K step r // 8 (the last four: the tail fragment)"""
    h = rec[limb * LIMB:(limb + 1) * LIMB].view(np.float16)
    steps = h[:4 * 512].reshape(4, 64, 8).transpose(0, 2, 1).reshape(32, 64)
    tail = h[4 * 512:].reshape(64, 4).T
    return np.concatenate([steps, tail]).astype(np.float64)


def _fragments(tile):
    """the fp32 fragment array [9][64][4] of a packed tile as [36 registers][64 lanes]"""
    return tile[:2304].reshape(9, 64, 4).transpose(0, 2, 1).reshape(36, 64).astype(np.float64)


@pytest.mark.parametrize('l', [0, 3])
def test_two_limb_records_decode_to_the_packed_weights(built, l):
    from disco_diffdock_amd.runtime import Context
    P = smr.random_conv_layer_params(CFG, l, 11 + l, True)
    ctx = {}
    for kernel in (0, 3):
        ctx[kernel] = Context(device=-1, conv_kernel=kernel)
        ctx[kernel].load_state_dict({f'conv_layers.{l}.{k}': v for k, v in P.items()})
    n_tiles = len(ctx[0].export(f'conv.{l}.tiles', np.int32)) // 4
    w2 = ctx[0].export(f'conv.{l}.w2x', np.uint32).view(np.uint8)
    w3 = ctx[3].export(f'conv.{l}.w2x', np.uint32).view(np.uint8)
    assert w2.size == (4 * n_tiles + 4) * REC2 and w3.size == (4 * n_tiles + 4) * REC3
    assert not w2[4 * n_tiles * REC2:].any()                                  # the zero pad records behind the last group
    scale = ctx[0].export(f'conv.{l}.xscale')
    assert np.array_equal(scale, ctx[3].export(f'conv.{l}.xscale'))
    for g in range(4):
        tiles = ctx[0].export(f'conv.{l}.w2p.{g}').reshape(n_tiles, -1)
        bias = ctx[0].export(f'conv.{l}.b2p.{g}').reshape(n_tiles, 32)
        for t in range(n_tiles):
            r2 = w2[(g * n_tiles + t) * REC2:][:REC2]
            r3 = w3[(g * n_tiles + t) * REC3:][:REC3]
            v = _fragments(tiles[t]) * float(scale[4 + g])
            hi, mid = _limb(r2, 0), _limb(r2, 1)
            assert np.array_equal(hi, v.astype(np.float32).astype(np.float16).astype(np.float64))
            assert (np.abs(hi + mid - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()      # the two-limb window pack_x3 checks
            assert np.array_equal(r2[:2 * LIMB], r3[:2 * LIMB])              # hi and mid: the three-limb record's bits
            back3 = hi + mid + _limb(r3, 2)                                  # three limbs: exact for |v| >= 0.5, within 2^-25 below
            assert (np.where(np.abs(v) >= 0.5, back3 == v, np.abs(back3 - v) <= 2.0 ** -25)).all()
            assert np.array_equal(r2[BIAS2:DESC2].view(np.float32), bias[t]) and np.array_equal(r2[BIAS2:DESC2], r3[BIAS3:DESC3])
            assert np.array_equal(r2[DESC2:DESC2 + 8], r3[DESC3:DESC3 + 8]) and not r2[DESC2 + 8:].any()
    # GEMM1: [group][3 row tiles][limbs x 4 608 B]
    a2 = ctx[0].export(f'conv.{l}.w1x', np.uint32).view(np.uint8).reshape(4, 3, 2 * LIMB)
    a3 = ctx[3].export(f'conv.{l}.w1x', np.uint32).view(np.uint8).reshape(4, 3, 3 * LIMB)
    assert np.array_equal(a2, a3[:, :, :2 * LIMB])
    for g in range(4):
        w1 = ctx[0].export(f'conv.{l}.w1p.{g}').reshape(3, -1)
        vmax = 0.0
        for T in range(3):
            v = _fragments(w1[T]) * float(scale[g])
            hi, mid = _limb(a2[g, T], 0), _limb(a2[g, T], 1)
            assert (np.abs(hi + mid - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()
            vmax = max(vmax, float(np.abs(v).max()))
        assert 2.0 ** 14 <= vmax < 2.0 ** 15          # the group's range scale
