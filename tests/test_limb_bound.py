"""The a-priori error bound of the default conv kernel's two-limb product (k_conv_x2.hip; DESIGN.md 3.3 "Round 6"), checked in numpy on the host: fp16 arithmetic of
numpy is IEEE round-to-nearest-even like v_cvt_f16_f32, products of fp16 numbers are exact in fp64 (and in the kernel's fp32 accumulator).  No GPU, no library call:
this pins the STATEMENT the kernel's accuracy claim rests on (models/tensor_layers.py:140-143,154-155 are plain fp32 GEMMs); the kernel itself is measured against
the fp64 oracle in tests/test_gpu_round6.py::test_two_limb_kernel_is_fp32_grade."""
import numpy as np
import pytest

from adversarial_operands import adversarial as _adversarial, range_scale as _range_scale, two_limbs as _two_limbs      # (moved: shared with the GPU test)
import adversarial_operands as adv


@pytest.mark.parametrize('binades', [3, 14, 30])
def test_two_limbs_carry_an_operand_to_2_to_the_minus_22(binades):
    rng = np.random.default_rng(5)
    x = _adversarial(rng, 72 * 4000, binades)
    xs = x.astype(np.float64) * _range_scale(x, 72)
    hi, mid = _two_limbs(xs)
    err = np.abs(xs - hi - mid)
    # relative 2^-22 wherever mid is a normal fp16 number (|x| >= 2^-3 after scaling), absolute 2^-25 (= 2^-39 of the group's maximum) below that
    assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(xs), 2.0 ** -25))
    assert np.all(np.abs(hi) < 65504) and np.all(np.abs(mid) <= 2.0 ** -11 * np.abs(xs) * (1 + 2.0 ** -10) + 2.0 ** -25)


def test_three_limb_products_stay_under_the_fp32_dot_product_bound():
    """hi.hi + hi.mid + mid.hi against the exact product: <= 3 * 2^-22 relative per product (two operand truncations + the dropped mid.mid), so a K = 72 dot
    product - plus the <= 14 roundings of its MFMA chain in the fp32 accumulator - stays under the classical a-priori bound 72 * 2^-24 * sum |a_i b_i| of an fp32 FMA
    chain of that length (what the reference's own fp32 GEMM guarantees)."""
    rng = np.random.default_rng(6)
    K, n = 72, 20000
    a = _adversarial(rng, n * K, 3)
    b = _adversarial(rng, n * K, 3)
    as_, bs_ = a.astype(np.float64) * _range_scale(a, K), b.astype(np.float64) * _range_scale(b, K)
    ah, am = _two_limbs(as_)
    bh, bm = _two_limbs(bs_)
    p3 = ah * bh + ah * bm + am * bh                         # exact in fp64: every term is a product of two 11-bit numbers
    exact = as_ * bs_
    rel = np.abs(p3 - exact) / np.abs(exact)
    assert rel.max() <= 3 * 2.0 ** -22 * (1 + 2.0 ** -9)
    assert rel.mean() < 2.0 ** -23                           # typical: a third of the bound
    dot3, dote, sabs = p3.reshape(n, K).sum(1), exact.reshape(n, K).sum(1), np.abs(exact).reshape(n, K).sum(1)
    trunc = np.abs(dot3 - dote) / sabs
    chain_roundings = 14 * 2.0 ** -24                        # one rounding per MFMA of the accumulator chain (each adds its K range exactly)
    assert trunc.max() + chain_roundings < 72 * 2.0 ** -24
    # ... and an fp32 FMA chain of the same operands, for scale: its error is of the same order (this is what `conv_kernel = 1` and the reference's CPU GEMM do)
    acc = np.zeros(n, dtype=np.float32)
    a2, b2 = as_.astype(np.float32).reshape(n, K), bs_.astype(np.float32).reshape(n, K)
    for k in range(K):
        acc = (acc.astype(np.float64) + a2[:, k].astype(np.float64) * b2[:, k].astype(np.float64)).astype(np.float32)      # fused multiply-add: one rounding per step
    chain = np.abs(acc.astype(np.float64) - dote) / sabs
    assert np.median(trunc) < 4 * np.median(chain) + 2.0 ** -26


@pytest.mark.parametrize('binades', [3, 14])
def test_emulated_kernel_arithmetic_is_at_least_as_accurate_as_an_fp32_fma_chain(binades):
    """The kernel's GEMM arithmetic restated bit for bit on the host - per K step of 16 the three MFMAs hi.mid, mid.hi, hi.hi into ONE fp32 accumulator (an MFMA adds the
    products of its K range exactly and rounds once), the packed K = 8 tail's two - against an fp32 FMA chain over the same 72 operands (one rounding per step: what
    `conv_kernel = 1` and the reference's CPU GEMM do), both against the exact dot product, on adversarial operands.  Relative to sum |a_i b_i|: the kernel's arithmetic is
    not worse than the chain at the median, the 99th percentile and the maximum (measured: median 1.27e-8 vs 1.35e-8, p99 5.5e-8 vs 8.6e-8, max 9.4e-8 vs 1.9e-7 at 3 binades)."""
    rng = np.random.default_rng(6 + binades)
    K, n = 72, 20000
    a, b = _adversarial(rng, n * K, binades), _adversarial(rng, n * K, binades)
    as_, bs_ = a.astype(np.float64) * _range_scale(a, K), b.astype(np.float64) * _range_scale(b, K)
    ah, am = [v.reshape(n, K) for v in _two_limbs(as_)]
    bh, bm = [v.reshape(n, K) for v in _two_limbs(bs_)]
    exact = (as_ * bs_).reshape(n, K)
    sabs, dote = np.abs(exact).sum(1), exact.sum(1)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    acc = np.zeros(n)
    for s in range(4):
        sl = slice(16 * s, 16 * s + 16)
        for A, B in ((ah, bm), (am, bh), (ah, bh)):                                    # X3_STEP of k_conv_x.hip under X3_TWO_LIMBS
            acc = f32(acc + (A[:, sl] * B[:, sl]).sum(1))
    sl = slice(64, 72)
    acc = f32(acc + (ah[:, sl] * bm[:, sl]).sum(1) + (am[:, sl] * bh[:, sl]).sum(1))      # X3_TAIL3: {W_hi, W_mid} x {h_mid, h_hi}
    acc = f32(acc + (ah[:, sl] * bh[:, sl]).sum(1) + (am[:, sl] * bm[:, sl]).sum(1))      #           {W_hi, W_mid} x {h_hi, h_mid}
    kern = np.abs(acc - dote) / sabs
    c = np.zeros(n, dtype=np.float32)
    a2, b2 = as_.astype(np.float32).reshape(n, K), bs_.astype(np.float32).reshape(n, K)
    for k in range(K):
        c = (c.astype(np.float64) + a2[:, k].astype(np.float64) * b2[:, k].astype(np.float64)).astype(np.float32)
    chain = np.abs(c.astype(np.float64) - dote) / sabs
    print(f'binades {binades}: kernel arithmetic median {np.median(kern):.2e} p99 {np.quantile(kern, .99):.2e} max {kern.max():.2e} | fp32 FMA chain median {np.median(chain):.2e} '
          f'p99 {np.quantile(chain, .99):.2e} max {chain.max():.2e}')
    assert np.median(kern) <= 1.05 * np.median(chain) and np.quantile(kern, .99) <= np.quantile(chain, .99) and kern.max() <= chain.max()
    assert kern.max() < 72 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------------------------
# the CPU companion of tests/test_gpu_conv_adversarial.py: the same layer inputs, the same bars, on the host restatement of the kernel arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', range(5))
def test_adversarial_layer_inputs_observe_every_weight_column_once(l):
    """What tests/test_gpu_conv_adversarial.py rests on, from the fp64 oracle: with one-hot senders, all-zero receivers with one edge each, a one-hot sh and an
    identity batch norm every output element of tp_conv_layer is ONE coefficient times ONE column of the radial MLP's output (adv.layout: differentiated AND
    confirmed by linearity); every one of the W columns is observed in every edge group; no element depends on two; the measures S cover exactly the non-zero
    elements, so nothing is excluded.  All four groups non-empty, no group size a multiple of 32, E <= 20 000."""
    L = adv.layout(l)
    assert all(n > 0 and n % 32 for n in adv.GROUP_SIZES) and sum(adv.GROUP_SIZES) <= 20000
    for arrangement, cls in (('gemm2', 'spread14'), ('gemm1', 'mixed_signs')):
        case = adv.make_case(l, arrangement, cls, 0)
        for g in range(4):
            obs = case['observed'][g]
            assert np.array_equal(obs[obs >= 0], np.arange(L['W'])), (l, g, 'a weight column is observed by no output element')
        ref = adv.oracle_output(case)
        E = case['splits'][-1]
        # the closed form (coefficient x one column of the fp64 MLP) IS the oracle's layer output, element for element
        P = {k: v.double().numpy() for k, v in case['P'].items()}
        want = np.zeros_like(ref)
        want[E:, :L['din']] = np.eye(L['din'])
        bn = (float(np.float32(1.0 - 1e-5)) + 1e-5) ** -0.5
        for g in range(4):
            a, b = case['splits'][g], case['splits'][g + 1]
            h = np.maximum(case['ea'][a:b].double().numpy() @ P[f'fc.{g}.0.weight'].T + P[f'fc.{g}.0.bias'], 0)
            w = h @ P[f'fc.{g}.4.weight'].T + P[f'fc.{g}.4.bias']
            c_of = L['col'][case['conf'][a:b]]
            want[a:b] = np.where(c_of >= 0, L['coef'][case['conf'][a:b]] * np.take_along_axis(w, np.maximum(c_of, 0), 1) * bn, 0.0)
        assert np.all(np.abs(want - ref) <= 1e-13 * case['S'] + 0.0), (l, arrangement)
        assert np.all((case['S'] > 0) == (np.pad(L['col'][case['conf']], ((0, L['din']), (0, 0)), constant_values=-1) >= 0))
        if arrangement == 'gemm2':
            assert min(case['hits']) == 1.0, case['hits']      # the packed W2 rows carry the class's bit patterns (adv.preimage)


@pytest.mark.parametrize('cls', adv.CLASSES)
@pytest.mark.parametrize('arrangement', ['gemm2', 'gemm1'])
def test_restated_kernel_meets_the_bars_on_adversarial_layer_inputs(arrangement, cls):
    """Bars (a) and (b) of adversarial_operands.py - the SAME GAMMA and floor constants the GPU test imports - on the host restatement of the default kernel's two
    GEMMs (K = 16 steps of three MFMAs plus the packed K = 8 tail, per-matrix / per-edge range scaling), and bar (a) on an fp32 FMA chain, for every operand
    class in both arrangements and both variants; layers 1 (n_in 30 / 30 / 6: the widest spread of row scales) and 3."""
    for l in (1, 3):
        for variant in (0, 1):
            case = adv.make_case(l, arrangement, cls, variant)
            assert case['scale_ok']
            ref = adv.oracle_output(case)
            f0 = adv.figures(adv.host_restatement(case), ref, case, 0)
            f1 = adv.figures(adv.host_restatement(case, chain=True), ref, case, 1)
            print(f'{arrangement} {cls} layer {l} variant {variant}: restated limbs {f0} | fma chain {f1}')
            assert f0['worst_over_bound'] <= 1.0, (l, variant, f0)
            assert f1['worst_over_bound'] <= 1.0, (l, variant, f1)


def test_the_bars_bite():
    """Each mutant of the restated arithmetic must break a bar on these operands: the hi.mid product dropped in ONE K step (bar (a), any class); mid converted
    with truncation (bar (b): the small-column class at 24 binades, where round-to-nearest loses 2^-29 and truncation 2^-24 per term, all of one sign);
    the range scale one binade up (hi overflows wherever a group's maximum sits one ulp under a power of two)."""
    def worst(arrangement, cls, mutant, l=3):
        case = adv.make_case(l, arrangement, cls, 0)
        return adv.figures(adv.host_restatement(case, mutant=mutant), adv.oracle_output(case), case, 0)['worst_over_bound']
    for arrangement in ('gemm2', 'gemm1'):
        assert worst(arrangement, 'spread3', None) <= 1.0
        assert worst(arrangement, 'spread3', 'drop_hi_mid_in_one_step') > 1.0
        assert worst(arrangement, 'mixed_signs', 'drop_hi_mid_in_one_step') > 1.0
        assert worst(arrangement, 'small_column', 'truncate_mid') > 1.0
        assert worst(arrangement, 'pow2_neighbours', 'scale_one_binade_up') > 1.0
    assert worst('gemm1', 'dominant_entry', 'truncate_mid') > 1.0
