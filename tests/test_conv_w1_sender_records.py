"""CPU test of the K = 48 GEMM1 records a host-only context packs for the default conv kernel's node-term split (conv_pack.hip: pack_x3; W1L_BYTES in
csrc/ddk_internal.h): [group][3 row tiles][hi | mid][3 K steps: [64 lanes][8 fp16]], exported as 'conv.<l>.w1sx'.  The kernel's B operand holds, in register
r' (0..23) of lane half hh, edge_emb[12 hh + r'] for r' < 12 and x_dst[12 hh + r' - 12] behind it; element i of K step s of lane (row + 32 hh) is register
8 s + i.  So every element is decoded and held against the column of fc.0.weight ([edge_emb | x_src | x_dst] x 24) its position stands for: first the 24
edge-embedding columns, then the 24 x_dst columns, and no x_src column anywhere (the positional comparison is exact; test_columns_cover... states the column set).  hi + mid must lie within max(2^-22 |v|, 2^-25) of the range-scaled weight.
A conv_kernel = 3 context has no such records and still exports the records it had."""
import numpy as np
import pytest

from oracle import score_model_ref as smr

CFG = smr.ScoreModelConfig()
NS, NE = 24, 72
LIMB = 3 * 1024                     # W1L_LIMB_BYTES
GROUP = 3 * 2 * LIMB                # W1L_BYTES
OLD_LIMB = 4 * 1024 + 512           # W2X_LIMB_BYTES: the K = 72 records


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


def _column(r, hh):
    """the column of fc.0.weight that register r of lane half hh multiplies"""
    return 12 * hh + r if r < 12 else 2 * NS + 12 * hh + (r - 12)


def test_columns_cover_edge_and_sender_blocks_only():
    cols = sorted(_column(r, hh) for r in range(24) for hh in range(2))
    assert cols == list(range(NS)) + list(range(2 * NS, 3 * NS))


@pytest.mark.parametrize('l', range(5))
def test_sender_records_decode_to_the_edge_and_x_dst_columns(built, l):
    from disco_diffdock_amd.runtime import Context
    P = smr.random_conv_layer_params(CFG, l, 23 + l, True)
    ctx = Context(device=-1, conv_kernel=0)
    ctx.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in P.items()})
    rec = ctx.export(f'conv.{l}.w1sx', np.uint32).view(np.uint8)
    assert rec.size == 4 * GROUP
    scale = ctx.export(f'conv.{l}.xscale')
    for g in range(4):
        W1 = P[f'fc.{g}.0.weight'].numpy().astype(np.float64)          # [72 hidden, 72 inputs]
        sc = float(scale[g])
        assert 2.0 ** 14 <= np.abs(W1).max() * sc < 2.0 ** 15          # the group's range scale (over all 72 columns, as for the K = 72 records)
        for T in range(3):
            base = g * GROUP + T * 2 * LIMB
            hi = rec[base:base + LIMB].view(np.float16).reshape(3, 64, 8).astype(np.float64)
            mid = rec[base + LIMB:base + 2 * LIMB].view(np.float16).reshape(3, 64, 8).astype(np.float64)
            want = np.zeros((3, 64, 8))
            for s in range(3):
                for lane in range(64):
                    hidden, hh = 32 * T + (lane & 31), lane >> 5
                    if hidden < NE:
                        want[s, lane] = [W1[hidden, _column(8 * s + i, hh)] * sc for i in range(8)]
            want = want.astype(np.float32).astype(np.float64)           # the packer scales in fp32 (a power of two: exact)
            assert np.array_equal(hi, want.astype(np.float32).astype(np.float16).astype(np.float64)), (g, T)
            assert (np.abs(hi + mid - want) <= np.maximum(2.0 ** -22 * np.abs(want), 2.0 ** -25)).all(), (g, T)
    ctx.close()


def test_conv_kernel_3_keeps_its_records(built):
    from disco_diffdock_amd.runtime import Context
    l = 1
    P = smr.random_conv_layer_params(CFG, l, 24, True)
    c0, c3 = Context(device=-1, conv_kernel=0), Context(device=-1, conv_kernel=3)
    for c in (c0, c3):
        c.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in P.items()})
    assert c3.export(f'conv.{l}.w1sx', np.uint32).size == 0             # the six-product form reads its K = 72 records
    a3 = c3.export(f'conv.{l}.w1x', np.uint32).view(np.uint8)
    a2 = c0.export(f'conv.{l}.w1x', np.uint32).view(np.uint8)
    assert a3.size == 4 * 3 * 3 * OLD_LIMB and a2.size == 4 * 3 * 2 * OLD_LIMB      # ... which both forms still export, unchanged
    assert np.array_equal(a2.reshape(4, 3, 2 * OLD_LIMB), a3.reshape(4, 3, 3 * OLD_LIMB)[:, :, :2 * OLD_LIMB])
    # the new records hold the same limb bits as registers 0..11 and 24..35 of the K = 72 records
    new = c0.export(f'conv.{l}.w1sx', np.uint32).view(np.uint8).reshape(4, 3, 2, LIMB)
    for g in range(4):
        for T in range(3):
            for limb in range(2):
                old = a2.reshape(4, 3, 2, OLD_LIMB)[g, T, limb].view(np.float16)
                steps = np.concatenate([old[:4 * 512].reshape(4, 64, 8).transpose(0, 2, 1).reshape(32, 64), old[4 * 512:].reshape(64, 4).T])      # [36 registers][64 lanes]
                got = new[g, T, limb].view(np.float16).reshape(3, 64, 8).transpose(0, 2, 1).reshape(24, 64)
                assert np.array_equal(got.view(np.uint16), np.concatenate([steps[:12], steps[24:36]]).view(np.uint16))
    for c in (c0, c3):
        c.close()
