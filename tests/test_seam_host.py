"""CPU: the host side of the joint sampling of overlapping windows: the float64 yardstick's fuse (tests/seam_ref.py),
the canvas noise of longform.noise_windows, the argument checks (raised before anything touches a device) and the
CLI flag."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_ref as SM      # noqa: E402


@pytest.fixture(scope="module")
def ldm():
    import models.model as M
    torch.manual_seed(0)
    return M.LDM(32, pretrained_path="").eval()


# ---- the yardstick's fuse --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,W,ov", [(3, 16, 1), (3, 16, 3), (3, 16, 8), (2, 64, 8)])
def test_fuse_follows_the_definition(B, W, ov):
    rng = np.random.default_rng(B * 100 + ov)
    x = rng.standard_normal((B, 5, 4, W))
    keep = x.copy()
    y = SM.fuse(x, ov)
    assert np.array_equal(x, keep)                                           # the input is left alone
    w = SM.weights(ov)
    assert np.array_equal(w, np.array([(j + 1) / (ov + 1) for j in range(ov)]))
    assert w[0] == 1.0 / (ov + 1) and w[-1] == ov / (ov + 1.0)               # the later window fades in, never 0 or 1
    touched = np.zeros(x.shape, dtype=bool)
    for b in range(B - 1):
        for j in range(ov):
            a, q = x[b, :, :, W - ov + j], x[b + 1, :, :, j]
            m = a + (j + 1) / (ov + 1) * (q - a)
            assert np.array_equal(y[b, :, :, W - ov + j], m)
            assert np.array_equal(y[b + 1, :, :, j], m)                      # both sides equal afterwards
        touched[b, :, :, W - ov:] = True
        touched[b + 1, :, :, :ov] = True
    assert np.array_equal(y[~touched], x[~touched])                          # elements outside the seams untouched
    assert np.array_equal(y[0, :, :, :W - ov], x[0, :, :, :W - ov])          # the first window's head has no seam
    assert np.array_equal(y[-1, :, :, ov:], x[-1, :, :, ov:])                # nor the last window's tail
    assert np.array_equal(SM.fuse(y, ov), y)                                 # a fused state is a fixed point


def test_fuse_of_one_window_is_the_identity_and_bad_widths_raise():
    x = np.random.default_rng(1).standard_normal((1, 3, 4, 16))
    assert np.array_equal(SM.fuse(x, 8), x)
    for ov in (0, 9, -1):
        with pytest.raises(ValueError):
            SM.fuse(np.zeros((2, 1, 1, 16)), ov)


# ---- the canvas noise ------------------------------------------------------------------------------------------------
def test_noise_windows_are_slices_of_one_canvas():
    from ldm_amd import longform as LF
    N, C, H, W, ov, seed = 5, 3, 4, 16, 4, 11
    nz = LF.noise_windows(N, C, H, W, ov, seed)
    want, canvas = SM.noise_windows(N, C, H, W, ov, seed)
    assert tuple(nz.shape) == (N, C, H, W) and nz.dtype == torch.float32 and nz.is_contiguous()
    assert tuple(canvas.shape) == (C, H, (N - 1) * (W - ov) + W)
    assert torch.equal(nz, want)
    for n in range(N):
        assert torch.equal(nz[n], canvas[:, :, n * (W - ov):n * (W - ov) + W])
    for n in range(N - 1):                                                   # neighbours share their overlap's noise
        assert torch.equal(nz[n, :, :, W - ov:], nz[n + 1, :, :, :ov])
    # independent of grouping: the windows are cut from the canvas, so any group of a call is a slice of them
    for bs in (1, 2, 3, 5):
        groups = [nz[b0:b0 + bs] for b0 in range(0, N, bs)]
        assert torch.equal(torch.cat(groups), nz)
    assert torch.equal(LF.noise_windows(N, C, H, W, ov, seed), nz)           # and repeatable
    assert not torch.equal(LF.noise_windows(N, C, H, W, ov, seed + 1), nz)
    for bad in (dict(ov=9), dict(ov=-1), dict(N=0)):
        kw = dict(N=N, C=C, H=H, W=W, ov=ov, seed=seed)
        kw.update(bad)
        with pytest.raises(ValueError):
            LF.noise_windows(**kw)


# ---- the argument checks ---------------------------------------------------------------------------------------------
def test_joint_value_errors(ldm):
    from models.transfer import HOP, transfer_recording
    content = torch.zeros(300 * HOP)
    with pytest.raises(ValueError, match="multiple of 8"):
        transfer_recording(ldm, content, content, frames=128, overlap=36, solver="dpmpp2m", num_timesteps=4, joint=True)
    with pytest.raises(ValueError, match="solver"):
        transfer_recording(ldm, content, content, frames=128, overlap=32, joint=True)
    x = torch.zeros(2, 1, 128, 128)
    with pytest.raises(ValueError, match="frames / 2"):
        ldm.content_style_transfer(x, x, steps=4, seam_overlap=72)
    with pytest.raises(ValueError, match="multiple of 8"):
        ldm.content_style_transfer(x, x, steps=4, seam_overlap=12)
    with pytest.raises(ValueError, match="solver"):
        ldm.content_style_transfer(x, x, steps=4, solver=None, seam_overlap=32)
    with pytest.raises(ValueError):
        ldm.content_style_transfer(x, x, steps=4, seam_overlap=-8)
    z = torch.zeros(2, 32, 16, 16)
    e = {"s5": torch.zeros(2, 256, 4, 4), "s6": torch.zeros(2, 512, 2, 2)}
    for bad in (9, -1, 2.5):
        with pytest.raises(ValueError, match="seam_cols"):
            ldm.style_conditioned_sample(z, e, steps=4, t_start=9, seam_cols=bad)


def test_cli_flag():
    from models.transfer import parse_args
    base = ["--content", "a.wav", "--style", "b.wav", "--out", "o.wav"]
    assert parse_args(base).joint is False
    a = parse_args(base + ["--solver", "dpmpp2m", "--joint"])
    assert a.joint is True and a.overlap == 64
    a = parse_args(base + ["--solver", "ddim", "--joint", "--overlap", "0", "--batch", "16"])
    assert a.joint is True and a.overlap == 0 and a.batch == 16
    for bad in (["--joint"],                                                 # needs --solver
                ["--solver", "dpmpp2m", "--joint", "--overlap", "60"]):      # not whole latent columns
        with pytest.raises(SystemExit):
            parse_args(base + bad)
