"""CPU test of the host reference of the transformer-tail fold (`hip.fold_linear_pair_ref`, what `ief_x3_fold_linear_pair` is held
against on the GPU): fp64 Wp W2, shapes, bias, and the identity the fold rests on."""
import numpy as np
import pytest
import torch

from ief_amd import hip


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("C,K", [(64, 256), (32, 96), (8, 8)])
def test_fold_reference_shapes_product_and_bias(C, K):
    wp, w2, b2, bp = _rand(C, C, seed=1) * C ** -0.5, _rand(C, K, seed=2) * K ** -0.5, _rand(C, seed=3), _rand(C, seed=4)
    wcat, bcat = hip.fold_linear_pair_ref(wp, w2, b2, bp)
    assert wcat.dtype == torch.float64 and bcat.dtype == torch.float64
    assert tuple(wcat.shape) == (C, K + C) and tuple(bcat.shape) == (C,)
    wp64, w264 = wp.numpy().astype(np.float64), w2.numpy().astype(np.float64)
    want = np.zeros((C, K))
    for j in range(C):                                  # the sum over j written out: no BLAS on this side
        want += wp64[:, j:j + 1] * w264[j:j + 1, :]
    assert np.abs(wcat[:, :K].numpy() - want).max() <= 1e-14 * np.abs(want).max()
    assert torch.equal(wcat[:, K:], wp.double()), "the second K range carries Wp itself"
    wantb = (wp64 * b2.numpy().astype(np.float64)[None, :]).sum(1) + bp.numpy().astype(np.float64)
    assert np.abs(bcat.numpy() - wantb).max() <= 1e-14 * np.abs(wantb).max()


def test_fold_reference_is_the_two_linears():
    C, K, M = 32, 96, 7
    wp, w2, b2, bp = _rand(C, C, seed=5), _rand(C, K, seed=6), _rand(C, seed=7), _rand(C, seed=8)
    g, h = _rand(M, K, seed=9).double(), _rand(M, C, seed=10).double()
    wcat, bcat = hip.fold_linear_pair_ref(wp, w2, b2, bp)
    two = (g @ w2.double().t() + b2.double() + h) @ wp.double().t() + bp.double()
    one = torch.cat([g, h], 1) @ wcat.t() + bcat
    assert (two - one).abs().max() <= 1e-12 * two.abs().max()


def test_fold_reference_without_biases_and_refusals():
    C, K = 8, 16
    wp, w2 = _rand(C, C, seed=11), _rand(C, K, seed=12)
    wcat, bcat = hip.fold_linear_pair_ref(wp, w2)
    assert float(bcat.abs().max()) == 0.0 and tuple(wcat.shape) == (C, K + C)
    _, only_bp = hip.fold_linear_pair_ref(wp, w2, None, _rand(C, seed=13))
    assert torch.equal(only_bp, _rand(C, seed=13).double())
    with pytest.raises(ValueError):
        hip.fold_linear_pair_ref(_rand(C, C + 1, seed=1), w2)
    with pytest.raises(ValueError):
        hip.fold_linear_pair_ref(wp, _rand(C + 1, K, seed=1))
