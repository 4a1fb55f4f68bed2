"""ba3c_amd.saliency's float64 statement of conv0's input gradient against torch's
conv_transpose2d of the un-pooled map, and its Toeplitz GEMM against the direct sum."""
import numpy as np
import pytest
import torch

from ba3c_amd import saliency as S
from oracle import ba3c_oracle as O

SHAPES = [(2, 8, 8), (1, 40, 40)]            # a pooled toy, one real-size image


def deal(seed, B, ph, pw, integers=False):
    rs = np.random.RandomState(seed)
    draw = (lambda size: rs.randint(-8, 9, size=size).astype(np.float64)) if integers else rs.normal
    c0 = rs.randint(0, 4, size=(B, ph, pw, 32)).astype(np.uint8)
    c0[rs.random_sample(c0.shape) < 0.3] = 255
    return draw(size=(B, ph, pw, 32)), c0, draw(size=(5, 5, 16, 32))


@pytest.mark.parametrize("B,ph,pw", SHAPES)
def test_the_rule_is_conv_transpose_of_the_unpooled_map(B, ph, pw):
    dp0, c0, w0 = deal(ph, B, ph, pw)
    dy = S.unpool_numpy(dp0, c0)
    live = c0 != 255
    assert np.array_equal(dy, O.maxpool2x2_backward(np.where(live, dp0, 0), np.where(live, c0, 0),
                                                    (2 * ph, 2 * pw)))
    ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(dy).permute(0, 3, 1, 2),
                                               torch.from_numpy(w0[:, :, :4]).permute(3, 2, 0, 1))
    got = S.conv0_input_grad_numpy(dp0, c0, w0)
    assert got.dtype == np.float64 and got.shape == (B, 2 * ph + 4, 2 * pw + 4, 4)
    np.testing.assert_allclose(got, ref.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12 * np.abs(got).max())
    assert np.array_equal(S.saliency_map(got), np.abs(got).sum(axis=3))


@pytest.mark.parametrize("B,ph,pw", SHAPES)
def test_the_toeplitz_gemm_is_the_direct_sum(B, ph, pw):
    """Small integers: every product and sum is exact in float64, so the two orders agree
    exactly; the padded channels 4..15 of the weights are read by neither."""
    dp0, c0, w0 = deal(100 + ph, B, ph, pw, integers=True)
    direct = S.conv0_input_grad_numpy(dp0, c0, w0)
    assert np.array_equal(S.conv0_input_grad_toeplitz(dp0, c0, w0), direct)
    w0[:, :, 4:] = 1e6
    assert np.array_equal(S.conv0_input_grad_toeplitz(dp0, c0, w0), direct)
