"""The bits of the pose update, the heads' finish and the bond rotor step: every output of se3_update, modify_conformer_batch, sample (plain, recorded,
no_torsion, guided), score_forward, randomize_position, conformer_rmsd and match_conformer on the cases of tests/golden/make_golden_pose_bits.py is
recomputed and its SHA-256 compared with tests/golden/pose_update_bits.json.  se3_update_kernel<POST, REC> and modify_conformer_batch_kernel run one
pose-update body, heads_post_kernel and the POST block one head finish, the rotor loop, match_eval and randomize_kernel one bond rotor step; the file
these kernels share is built with floating-point contraction on, so that the same text gives the same bits in every kernel is a property of the build.
The fp64 tests hold these outputs to fp32 grade and would see nothing of a multiply-add contracted differently in one of them.  This test does.

The file pins this toolchain: ``sinf`` / ``cosf`` / ``tanhf`` / ``expf`` come from the device library, and which multiply-adds are fused is the
compiler's choice.  After a ROCm change the file is regenerated (the generator's docstring) from a commit known to be good, never from the commit under
test.  A missing entry is a failure, not a skip: an output without a pinned digest is an unchecked output."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_pose_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRIES = ('se3_update', 'batch', 'sample', 'sample_no_torsion', 'guided', 'score', 'randomize', 'rmsd', 'match')


@pytest.fixture(scope='module')
def got():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return gen.digests(torch.device('cuda:0'))


@pytest.fixture(scope='module')
def want():
    with open(os.path.join(GOLDEN, 'pose_update_bits.json')) as f:
        return json.load(f)['sha256']


def test_every_output_is_pinned(got, want):
    assert sorted(got) == sorted(want)
    assert {k.split('.')[0] for k in want} == set(ENTRIES)


@pytest.mark.parametrize('entry', ENTRIES)
def test_bits(got, want, entry):
    names = [k for k in got if k.split('.')[0] == entry]
    assert names, entry
    missing = [k for k in names if k not in want]
    assert not missing, missing
    changed = [k for k in names if got[k] != want[k]]
    print(entry, f'{len(names)} outputs, {len(changed)} changed')
    assert not changed, changed
