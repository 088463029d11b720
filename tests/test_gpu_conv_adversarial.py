"""The conv kernels (ddk_conv_forward, conv_kernel 0 / 1 / 3) on adversarial radial-MLP operands, per weight column, against the fp64 oracle's tp_conv_layer.

tests/adversarial_operands.py builds layer inputs in which every output element is one tensor-product coefficient times ONE dot product of the radial MLP
(confirmed from the oracle by tests/test_limb_bound.py::test_adversarial_layer_inputs_observe_every_weight_column_once, with 100 % of the weight columns of
every layer and edge group observed), fills the two GEMMs' operands with the values that make the fp16 limb roundings worst-case, and states the bars; its
docstring derives them term by term.  In short, with u = 2^-24, S = sum_k |W'_ck h_k| + |b'_c| of the observed column and kappa its coefficient:
  (a) |kernel - fp64| <= |kappa| GAMMA S,  GAMMA = 89 u (1 + 2^-10) = (3 packing + 73 dot product and bias + 5 pass-through GEMM + 6 coefficient + 2 mean and batch
      norm) u: kernel 1 in every class; kernels 0 and 3 wherever every operand lies within 17 binades of its range-scaling group's maximum;
  (b) |kernel - fp64| <= |kappa| (GAMMA S + FLOOR),  FLOOR = 2^-39 (1 + 2^-9) (M_W sum |h_k| + N_H M_h sum |W'_ck|) + 72 * 2^-78 M_W M_h (+ 2^-39 (1 + 2^-9) M_hid
      in the `gemm1` arrangement): kernels 0 and 3 in the 30-binade, small-column and dominant-entry classes - from |x - hi - mid| <= max(2^-22 |x|, 2^-25) after
      scaling a group's maximum M into [2^14, 2^15);
  (c) in the 3- and 14-binade classes the default's max and p99 of error / (|kappa| S) <= 1.5 x kernel 1's on the same operands, no additive term.
Elements that depend on no weight column (and the senders' own rows) must be reproduced exactly.  The same bars hold on the host restatement of the kernel
arithmetic, and mutants of it break them (tests/test_limb_bound.py).  Every Context names its conv_kernel, so the file means the same under DDK_CONV_KERNEL /
DDK_DETERMINISTIC.  Figures are kept through _record_drift (keys conv_adversarial_layer_<l>_kernel_<k>_<class>)."""
import numpy as np
import pytest
import torch

import adversarial_operands as adv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.mark.parametrize('l', range(5))
def test_conv_kernels_on_adversarial_operands_per_weight_column(dev, l):
    from disco_diffdock_amd.runtime import Context
    from test_gpu_round3 import _record_drift
    L = adv.layout(l)
    failures = []
    for cls in adv.CLASSES:
        rel = {k: [] for k in (0, 1, 3)}
        worst = {k: 0.0 for k in (0, 1, 3)}
        for arrangement in ('gemm2', 'gemm1'):
            for variant in (0, 1):
                case = adv.make_case(l, arrangement, cls, variant)
                assert case['scale_ok']
                ref = adv.oracle_output(case)
                s = case['splits']
                args = (l, case['node'].to(dev), case['ei'][0].to(dev), case['ei'][1].to(dev), s, case['ea'].to(dev), case['sh'].to(dev), L['dout'])
                obs = case['S'] > 0
                for kernel in (0, 1, 3):
                    ctx = Context(device=0, conv_kernel=kernel)
                    assert int(ctx.cfg.conv_kernel) == kernel
                    ctx.load_state_dict({f'conv_layers.{l}.{k}': v for k, v in case['P'].items()})
                    out = ctx.conv_forward(*args).cpu().numpy()
                    f = adv.figures(out, ref, case, kernel)
                    err = np.abs(out.astype(np.float64) - ref)
                    rel[kernel].append(np.where(np.isfinite(err[obs]), err[obs], np.inf) / case['S'][obs])
                    worst[kernel] = max(worst[kernel], f['worst_over_bound'])
                    print(f'layer {l} {cls} {arrangement} variant {variant} kernel {kernel}: error / S max {f["max"]:.3e} p99 {f["p99"]:.3e}, '
                          f'worst error / bound {f["worst_over_bound"]:.3f}')
                    if not f['worst_over_bound'] <= 1.0:
                        failures.append(('bar (b)' if kernel != 1 and cls in adv.FLOOR_CLASSES else 'bar (a)', cls, arrangement, variant, kernel, f))
        fig = {}
        for kernel in (0, 1, 3):
            r = np.concatenate(rel[kernel])
            fig[kernel] = (float(r.max()), float(np.quantile(r, 0.99)))
        for kernel in (0, 1, 3):
            _record_drift(f'conv_adversarial_layer_{l}_kernel_{kernel}_{cls}', fig[kernel][0], bar=adv.GAMMA, max_err_over_S=fig[kernel][0], p99_err_over_S=fig[kernel][1],
                          max_ratio_to_kernel_1=fig[kernel][0] / fig[1][0], p99_ratio_to_kernel_1=fig[kernel][1] / fig[1][1],
                          headroom_under_gamma=adv.GAMMA / fig[kernel][0], worst_error_over_bound=worst[kernel],
                          bound='a' if kernel == 1 or cls not in adv.FLOOR_CLASSES else 'b')
        print(f'layer {l} {cls}: default / kernel 1 ratio of error / S: max {fig[0][0] / fig[1][0]:.3f} p99 {fig[0][1] / fig[1][1]:.3f}')
        if cls in adv.RATIO_CLASSES and not (fig[0][0] <= adv.RATIO_C * fig[1][0] and fig[0][1] <= adv.RATIO_C * fig[1][1]):
            failures.append(('bar (c)', cls, fig))
    assert not failures, failures
