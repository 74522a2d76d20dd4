"""CPU checks of tests/mxfp4_hadamard_ref.py, the restatement the GPU tests hold the rotated quantisers to."""
import pytest
import torch

import mxfp4_hadamard_ref as HR


@pytest.mark.parametrize("D", [64, 128, 256])
def test_transform_is_the_sylvester_matrix_and_its_own_inverse_times_d(D):
    """On small integers every stage is exact: H x equals the matrix product and H (H x) = D x, bit for bit."""
    x = torch.randint(-8, 9, (5, D), generator=torch.Generator().manual_seed(D)).float()
    i = torch.arange(D)
    H = 1.0 - 2.0 * torch.tensor([[bin(a & b).count("1") & 1 for b in i.tolist()] for a in i.tolist()])
    y = HR.hadamard(x)
    assert torch.equal(y, x @ H) and torch.equal(HR.hadamard(y), D * x)
