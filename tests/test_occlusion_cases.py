"""CPU check of the input sets of tests/test_gpu_occlusion.py (tests/occlusion_cases.py): on the oracle's mask alone, every set contains what
it is there for (who must be hidden and who must not), and the random crowds are neither all visible nor all hidden."""
import pytest

import occlusion_cases as oc


@pytest.mark.parametrize('B,A,E,name', oc.cases(), ids=lambda v: str(v))
def test_set_holds_what_it_claims(oracle, B, A, E, name):
    state, size, present, marks = oc.make(B, A, E, name)
    mask = oracle.occlusion_mask(state, size, present, A)
    oc.check_conditions(B, A, E, name, state, size, present, marks, mask)
