"""Step kernels (csrc/uconv.hip) of the reverse loop: every layer against float64 torch, and the whole
loop on them against the general-kernel loop and the oracle.

Tolerance: 1e-5 relative (max-norm) per layer against float64 — fp32 MFMA accumulation in a different
order than torch; the loop to 1e-5 against the general kernels and 1e-4 (north_star) against the oracle.
Reference: model.py:178-194 (layers), :205-229 (epilogue order: ReLU, then + t_emb / + skip),
:409-465 (loop).
"""
import pytest
import torch

import recipe
from conftest import rel_err
from step_ref import check_step_layer, npy

pytestmark = pytest.mark.gpu


def _case(variant, layer, shape):
    return variant, layer, shape


@pytest.mark.parametrize("variant,layer,shape",
                         [_case("uconv", l, s) for l in range(8) for s in [(8, 16, 64), (2, 16, 16), (3, 8, 24)]] +
                         [_case("ksplit", l, s) for l in (2, 3, 4, 5, 6) for s in [(8, 16, 64), (2, 16, 16), (3, 8, 24),
                                                                                  (5, 16, 64)]])
def test_step_layer_vs_float64(cuda, variant, layer, shape):
    """uconv: ldm_step_conv (register-direct, any latent with H, W multiples of 8); ksplit: ldm_step_conv_ws
    (the same kernel with 32x32 tiles and K split over blocks).  The split form runs twice on one workspace:
    bitwise-equal results (the split-K sum is in slot order) and the counters left zero."""
    check_step_layer(cuda, variant, layer, shape)


@pytest.mark.parametrize("shape,eta", [((8, 16, 64), 0.0), ((2, 16, 16), 1.0), ((3, 8, 24), 0.4), ((1, 16, 64), 0.0),
                                       ((4, 16, 64), 0.7)])
def test_step_loop_equals_general_loop(M, cuda, shape, eta):
    """The reverse loop on the step kernels (NHWC state, fused dec1 update; use_step 1 and 2 =
    uconv.hip) == the same folded loop on conv.hip's general kernel, final x and
    both logs."""
    from ldm_amd.engine import UNetEngine
    B, H, W = shape
    unet = M.UNet(32, 32, 64)
    recipe.fill_module(unet, seed=100)
    unet = unet.to(cuda)
    fd = M.ForwardDiffusion(200)
    times = torch.linspace(199, 0, 6).long()
    coefs = fd.reverse_coefs(times).to(cuda)
    x0 = torch.from_numpy(recipe.normal((B, 32, H, W), 41)).to(cuda)
    s5 = torch.from_numpy(recipe.uniform01((B, 256, H // 4, W // 4), 42)).to(cuda)
    s6 = torch.from_numpy(recipe.uniform01((B, 512, H // 8, W // 8), 43)).to(cuda)
    tt = times[:-1].view(-1, 1).expand(-1, B).contiguous().to(cuda)
    outs = []
    with torch.no_grad():
        for step in (0, 1, 2):   # (2: the nine layers share one split-K workspace)
            eng = UNetEngine(unet, fold=True, step=step)
            x = x0.clone()
            lg = (torch.empty((5, B, 32, H, W), device=cuda), torch.empty((5, B, 32, H, W), device=cuda))
            eng.ddim_loop(x, s5, s6, tt, coefs, eta, *lg)
            assert eng.weights(eng.shape(B, 32, H, W)).use_step == step
            outs.append((x, lg[0], lg[1]))
    torch.cuda.synchronize()
    for k in (1, 2):
        for a, b in zip(outs[0], outs[k]):
            assert rel_err(npy(b), npy(a)) < 1e-5


@pytest.fixture(scope="module")
def M():
    import models.model as M
    return M
