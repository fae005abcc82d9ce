"""
tds_occlusion_mask_f32 against the CPU oracle (oracle.occlusion_mask: the same operation order, anchored to the reference's masks by
tests/test_observation.py), exactly, at the entity counts where the 64-target chunk loop wraps and on hand-placed edge cases: collinear,
coincident, tangent, zero-width, absent and NaN entities (tests/occlusion_cases.py; tests/test_occlusion_cases.py checks the sets on the CPU).
"""
import numpy as np
import pytest
import torch

import occlusion_cases as oc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.mark.parametrize('B,A,E,name', oc.cases(), ids=lambda v: str(v))
def test_occlusion_mask_matches_oracle(oracle, B, A, E, name):
    from torchdrivesim_amd import _ops
    state, size, present, marks = oc.make(B, A, E, name)
    ref = oracle.occlusion_mask(state, size, present, A)
    oc.check_conditions(B, A, E, name, state, size, present, marks, ref)
    out = _ops.occlusion_mask(torch.from_numpy(state).to(DEV), torch.from_numpy(size).to(DEV), torch.from_numpy(present).to(DEV), A)
    assert out.dtype == torch.bool and out.shape == (B, A, E)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
