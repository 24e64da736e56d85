"""CPU: the regional keep's host side: the coefficient table, the mask builders, the reduction to latent resolution,
the argument checks (raised before anything touches a device), the CLI flags and the float64 yardstick
(tests/regional_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regional_ref as RR      # noqa: E402
import solver_ref as SR        # noqa: E402


@pytest.fixture(scope="module")
def ldm():
    import models.model as M
    torch.manual_seed(0)
    return M.LDM(32, pretrained_path="").eval()


def emb(B=2, H=16, W=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"s5": torch.rand(B, 256, H // 4, W // 4, generator=g), "s6": torch.rand(B, 512, H // 8, W // 8, generator=g)}


# ---- keep_coefs ------------------------------------------------------------------------------------------------------
def test_keep_coefs_are_reverse_coefs_columns(ldm):
    fd = ldm.noise_scheduler
    times = torch.from_numpy(SR.sample_times(99, 5))
    rc = fd.reverse_coefs(times)
    kc = fd.keep_coefs(times, exact_last=False)
    assert kc.dtype == torch.float32 and tuple(kc.shape) == (5, 2) and kc.is_contiguous()
    assert torch.equal(kc, rc[:, 2:4])
    ke = fd.keep_coefs(times)
    assert torch.equal(ke[:-1], rc[:-1, 2:4]) and ke[-1].tolist() == [1.0, 0.0]
    assert torch.equal(rc, fd.reverse_coefs(times))      # (the table it is cut from is not written to)
    want = RR.keep_coefs(SR.alpha_bar(ldm.num_timesteps), SR.sample_times(99, 5))
    assert np.abs(ke.double().numpy() - want).max() <= 1e-6


def test_yardstick_endpoints():
    """A check of the yardstick itself (tests/regional_ref.py), not of the code under test: w = 0 is the plain float64
    loop, w = 1 ends on the content's trajectory whatever the denoiser says."""
    import guidance_ref as GR
    ab, times = SR.alpha_bar(200), SR.sample_times(99, 4)
    rng = np.random.default_rng(0)
    x, z0, n0 = (rng.standard_normal((2, 3, 4, 5)) for _ in range(3))
    eps = lambda xv, i: np.tanh(xv) * (i + 1)      # noqa: E731
    for solver, eta in (("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m", 0.0)):
        c = RR.keep_coefs(ab, times)
        p, p0, pe = GR.plain(ab, times, x, eps, solver, eta)
        k, k0, ke = RR.solve(ab, times, x, eps, z0, n0, np.zeros((2, 4, 5)), c, solver, eta)
        assert np.array_equal(k, p) and all(np.array_equal(u, v) for u, v in zip(k0 + ke, p0 + pe))
        k, _, _ = RR.solve(ab, times, x, eps, z0, n0, np.ones((2, 4, 5)), c, solver, eta)
        assert np.array_equal(k, z0)
        c = RR.keep_coefs(ab, times, exact_last=False)
        k, _, _ = RR.solve(ab, times, x, eps, z0, n0, np.ones((2, 4, 5)), c, solver, eta)
        assert np.array_equal(k, RR.known(z0, n0, c[-1][0], c[-1][1]))


def test_kept_region_follows_a_perfect_denoiser_under_ddim():
    """Again the yardstick only, in float64: with x = q_sample(z0, t, n0) and a denoiser that returns n0, DDIM (eta 0)
    lands on a_i z0 + b_i n0 after every step, the trajectory the kept region is held on.  The next test checks the
    same on the fp32 tables of the code under test."""
    import guidance_ref as GR
    ab, times = SR.alpha_bar(200), SR.sample_times(99, 4)
    rng = np.random.default_rng(1)
    z0, n0 = rng.standard_normal((2, 3, 4, 5)), rng.standard_normal((2, 3, 4, 5))
    x = np.sqrt(ab[times[0]]) * z0 + np.sqrt(1 - ab[times[0]]) * n0
    c = RR.keep_coefs(ab, times, exact_last=False)
    for i in range(4):
        x, _ = GR.ddim_step(ab, times, i, x, n0, 0.0)
        assert np.abs(x - RR.known(z0, n0, c[i][0], c[i][1])).max() <= 1e-12


def test_kept_region_is_the_fp32_ddim_trajectory(ldm):
    """The same property on the fp32 tables the device reads: x = q_sample(z0, t, n0), the reference's update
    (ddim_update's op sequence, eta 0) on eps = n0 with reverse_coefs, against keep_blend's `known` on keep_coefs.  Both
    are fp32 with one rounding per operation, so they agree to a few ulp of the values at every step."""
    fd = ldm.noise_scheduler
    times = torch.from_numpy(SR.sample_times(99, 4))
    rc, kc = fd.reverse_coefs(times), fd.keep_coefs(times, exact_last=False)
    g = torch.Generator().manual_seed(2)
    z0, n0 = torch.randn(2, 3, 4, 5, generator=g), torch.randn(2, 3, 4, 5, generator=g)
    x = rc[0, 0] * z0 + rc[0, 1] * n0
    for i in range(4):
        sat, s1t, san, s1n = rc[i]
        x0 = (x - s1t * n0) / sat
        x = san * x0 + s1n * n0
        known = kc[i, 0] * z0 + kc[i, 1] * n0
        assert float((x - known).abs().max()) <= 8 * 2.0 ** -23 * float(known.abs().max())
    # with exact_last the last row drops the noise term altogether
    ke = fd.keep_coefs(times)
    assert torch.equal(ke[-1, 0] * z0 + ke[-1, 1] * n0, z0)


def test_transfer_mask_is_checked_before_anything_runs(ldm):
    """content_style_transfer validates shape, finiteness and range of the mask first, before the encoder or the
    sampler are reached."""
    xc, xs = torch.rand(2, 1, 128, 128), torch.rand(2, 1, 128, 128)
    bad = torch.zeros(2, 1, 128, 128)
    bad[1, 0, 5, 5] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        ldm.content_style_transfer(xc, xs, keep=bad)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        ldm.content_style_transfer(xc, xs, keep=torch.full((2, 1, 128, 128), 1.5))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        ldm.content_style_transfer(xc, xs, keep=torch.full((2, 16, 16), -0.5))
    with pytest.raises(ValueError, match="n_mels,F"):
        ldm.content_style_transfer(xc, xs, keep=torch.zeros(2, 1, 64, 128))
    with pytest.raises(ValueError, match="latent-resolution"):
        ldm.content_style_transfer(xc, xs, keep=torch.zeros(2, 16, 8))


# ---- keep_mask / mask_windows / latent_keep --------------------------------------------------------------------------
def test_keep_mask_times_bands_feather_union():
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    sr, hop, T, M = 22050, A.N_FFT // 4, 40, 128
    z = LF.keep_mask(T, M, sr)
    assert z.dtype == torch.float32 and tuple(z.shape) == (M, T) and not z.is_cuda and float(z.abs().max()) == 0.0
    # frames 10 .. 20 (frame f stands at f * hop / sr seconds)
    t0, t1 = 10 * hop / sr, 20 * hop / sr + 1e-9
    m = LF.keep_mask(T, M, sr, times=[(t0, t1)])
    want = torch.zeros(M, T)
    want[:, 10:21] = 1
    assert torch.equal(m, want)
    # a feather of 3 frames inside each edge: 1/4, 2/4, 3/4, then 1
    m = LF.keep_mask(T, M, sr, times=[(t0, t1)], feather=3)
    assert m[0, 9:25].tolist() == [0, 0.25, 0.5, 0.75, 1, 1, 1, 1, 1, 0.75, 0.5, 0.25, 0, 0, 0, 0]
    assert torch.equal(m, m[:1].expand(M, T))
    # a span from the start of the recording: no ramp at the recording's own end
    m = LF.keep_mask(T, M, sr, times=[(0.0, t0)], feather=3)
    assert m[5, :13].tolist() == [1] * 8 + [0.75, 0.5, 0.25, 0, 0]
    # a band: the bins whose centre frequency lies in it
    fc = A.mel_centre_frequencies(sr, M)
    assert fc.shape == (M,) and np.all(np.diff(fc) > 0) and 0 < fc[0] and fc[-1] < sr / 2
    b = LF.keep_mask(T, M, sr, bands=[(0.0, 200.0)])
    nb = int((fc <= 200.0).sum())
    assert 0 < nb < M and torch.equal(b[:, 3], torch.tensor([1.0] * nb + [0.0] * (M - nb)))
    bf = LF.keep_mask(T, M, sr, bands=[(0.0, 200.0)], feather=1)
    assert bf[nb - 1, 0] == 0.5 and bf[nb - 2, 0] == 1.0 and bf[0, 0] == 1.0
    # the union is the maximum
    u = LF.keep_mask(T, M, sr, times=[(t0, t1), (30 * hop / sr, 99.0)], bands=[(0.0, 200.0)], feather=3)
    parts = [LF.keep_mask(T, M, sr, times=[(t0, t1)], feather=3), LF.keep_mask(T, M, sr, times=[(30 * hop / sr, 99.0)], feather=3),
             LF.keep_mask(T, M, sr, bands=[(0.0, 200.0)], feather=3)]
    assert torch.equal(u, torch.stack(parts).amax(0))
    assert float(u.min()) >= 0 and float(u.max()) <= 1
    with pytest.raises(ValueError):
        LF.keep_mask(T, M, sr, times=[(2.0, 1.0)])
    with pytest.raises(ValueError):
        LF.keep_mask(T, M, sr, feather=-1)


def test_mask_windows_follows_the_window_plan():
    from ldm_amd import longform as LF
    T, frames, overlap = 300, 128, 32      # stride 96: windows at 0, 96, 192; the last one is padded from 300 on
    N, stride = LF.window_plan(T, frames, overlap)
    assert (N, stride) == (3, 96) and (N - 1) * stride + frames > T
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(16, T, generator=g)
    mw = LF.mask_windows(mask, frames, overlap)
    assert tuple(mw.shape) == (N, 1, 16, frames)
    for n in range(N):
        t0 = n * stride
        live = min(frames, T - t0)
        assert torch.equal(mw[n, 0, :, :live], mask[:, t0:t0 + live])
        assert float(mw[n, 0, :, live:].abs().sum()) == 0.0
    assert live < frames
    with pytest.raises(ValueError):
        LF.mask_windows(mask[0], frames, overlap)


def test_latent_keep_is_the_cell_mean():
    import models.model as M
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(2, 1, 32, 48, generator=g)
    got = M.LDM.latent_keep(mask)
    assert tuple(got.shape) == (2, 4, 6) and got.dtype == torch.float32
    want = mask.double().numpy().reshape(2, 4, 8, 6, 8).mean(axis=(2, 4))
    assert np.abs(got.double().numpy() - want).max() <= 1e-6
    assert torch.equal(M.LDM.latent_keep(torch.ones(1, 1, 16, 16)), torch.ones(1, 2, 2))
    with pytest.raises(ValueError):
        M.LDM.latent_keep(torch.rand(2, 1, 30, 48))
    with pytest.raises(ValueError):
        M.LDM.latent_keep(torch.rand(2, 32, 48))


# ---- the argument checks ---------------------------------------------------------------------------------------------
def test_keep_value_errors(ldm):
    from ldm_amd.engine import UNetEngine
    B, C, H, W, n = 2, 32, 16, 16, 3
    z = torch.zeros(B, C, H, W)
    z0, n0, w, coefs = torch.zeros_like(z), torch.zeros_like(z), torch.full((B, H, W), 0.5), torch.zeros(n, 2)
    ok = UNetEngine.keep_operands((z0, n0, w, coefs), z.shape, n, "cpu")
    assert len(ok) == 4 and all(t.dtype == torch.float32 and t.is_contiguous() for t in ok)
    assert UNetEngine.keep_operands(ok, z.shape, n, "cpu") is ok
    assert len(UNetEngine.keep_operands(dict(z0=z0, n0=n0, w=w, coefs=coefs), z.shape, n, "cpu")) == 4
    for bad in (torch.full((B, H, W), 1.5), torch.full((B, H, W), -0.1)):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            UNetEngine.keep_operands((z0, n0, bad, coefs), z.shape, n, "cpu")
    nan = w.clone()
    nan[1, 2, 3] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        UNetEngine.keep_operands((z0, n0, nan, coefs), z.shape, n, "cpu")
    for args in ((z0[:1], n0, w, coefs), (z0, n0[:, :8], w, coefs), (z0, n0, w[:, :8], coefs), (z0, n0, w.unsqueeze(1), coefs),
                 (z0, n0, w, coefs[:2]), (z0, n0, w, torch.zeros(n, 4))):
        with pytest.raises(ValueError):
            UNetEngine.keep_operands(args, z.shape, n, "cpu")
    with pytest.raises(ValueError):
        UNetEngine.keep_operands(dict(z0=z0, n0=n0, w=w), z.shape, n, "cpu")
    # through the public sampler, before anything runs
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        ldm.style_conditioned_sample(z, emb(), steps=n, t_start=9, keep=torch.full((B, H, W), 2.0), z0=z0, noise=n0)
    with pytest.raises(ValueError, match="finite"):
        ldm.style_conditioned_sample(z, emb(), steps=n, t_start=9, keep=nan, z0=z0, noise=n0)
    with pytest.raises(ValueError, match="z0"):
        ldm.style_conditioned_sample(z, emb(), steps=n, t_start=9, keep=w)
    with pytest.raises(ValueError):
        ldm.style_conditioned_sample(z, emb(), steps=n, t_start=9, keep=w[:, :8], z0=z0, noise=n0)


def test_keep_without_a_solver_raises(ldm):
    from models.transfer import HOP, transfer_recording
    content = torch.zeros(40 * HOP)
    keep = torch.zeros(128, 41)
    with pytest.raises(ValueError, match="solver"):
        transfer_recording(ldm, content, content, keep=keep)
    with pytest.raises(ValueError, match="n_mels, T_total"):
        transfer_recording(ldm, content, content, keep=keep[:, :40], solver="dpmpp2m", num_timesteps=4)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        transfer_recording(ldm, content, content, keep=keep + 2, solver="dpmpp2m", num_timesteps=4)


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from models.transfer import parse_args
    base = ["--content", "a.wav", "--style", "b.wav", "--out", "o.wav"]
    a = parse_args(base)
    assert a.keep_time == [] and a.keep_band == [] and a.keep_feather == 0 and a.composite is True
    a = parse_args(base + ["--solver", "dpmpp2m", "--keep-time", "0:10", "--keep-time", "42.5:60", "--keep-band", "0:200",
                           "--keep-feather", "8", "--no-composite"])
    assert a.keep_time == [(0.0, 10.0), (42.5, 60.0)] and a.keep_band == [(0.0, 200.0)]
    assert a.keep_feather == 8 and a.composite is False
    for bad in (["--keep-time", "0:10"],                                   # needs --solver
                ["--solver", "ddim", "--keep-time", "10:0"], ["--solver", "ddim", "--keep-band", "abc"],
                ["--solver", "ddim", "--keep-time", "1:2:3"], ["--solver", "ddim", "--keep-feather", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
