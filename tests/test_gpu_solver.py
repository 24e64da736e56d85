"""GPU: the multistep sampler (DPM-Solver++(2M), first-order first and last step) from the stand-alone update kernel
up to transfer_recording, against the float64 yardstick tests/solver_ref.py (lambda / h / r form) and the oracle's UNet.
1e-5 relative for the fp32 update (as test_gpu_bench_config.py holds the DDIM update to), 1e-4 for whole-UNet parity."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR       # noqa: E402
import solver_ref as SR      # noqa: E402

pytestmark = pytest.mark.gpu
UPD_TOL, PARITY_TOL = 1e-5, 1e-4


def npy(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def ctx(cuda):
    """The model (never modified), its float64 state dict and schedule."""
    import models.model as M
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm.state_dict().items()}
    return dict(M=M, ldm=ldm, sd64=sd64, ab=SR.alpha_bar(ldm.num_timesteps))


def inputs(B, H, W, seed, C=32):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g)
    s5 = torch.rand(B, 256, H // 4, W // 4, generator=g)
    s6 = torch.rand(B, 512, H // 8, W // 8, generator=g)
    return z, s5, s6


def table64(coef):
    return coef.double().cpu().numpy()


def upd64(c, x, eps, prev):
    """One row of the table in float64 (c: the fp32 row the kernel reads, widened)."""
    x0 = (x - c[1] * eps) / c[0]
    return c[2] * x + c[3] * x0 + (c[4] * prev if prev is not None else 0.0), x0


# ---- the stand-alone step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prev", [False, True])
def test_msolver_step_matches_float64(ctx, cuda, with_prev):
    from ldm_amd import ops
    fd = ctx["ldm"].noise_scheduler
    coef = fd.multistep_coefs(SR.sample_times(99, 10))[3].contiguous()      # a second-order row
    assert float(coef[4]) != 0.0
    g = torch.Generator().manual_seed(5)
    x, eps, prev = (torch.randn(2, 32, 8, 8, generator=g) for _ in range(3))
    xd = x.to(cuda)
    x0l = torch.full_like(xd, float("nan"))
    epl = torch.full_like(xd, float("nan"))
    ops.msolver_step_(xd, eps.to(cuda), coef.to(cuda), x0l, prev.to(cuda) if with_prev else None, epl)
    torch.cuda.synchronize()
    xn, x0 = upd64(table64(coef), npy(x), npy(eps), npy(prev) if with_prev else None)
    e1, e2 = rel_err(npy(xd), xn), rel_err(npy(x0l), x0)
    print(f"with_prev {with_prev}: x {e1:.2e}, x0 {e2:.2e}")
    assert e1 <= UPD_TOL and e2 <= UPD_TOL
    assert torch.equal(epl.cpu(), eps)
    with pytest.raises(ValueError):
        ops.msolver_step_(xd, eps.to(cuda), coef.to(cuda), None)


def test_gaussian_model_through_the_kernel(ctx, cuda):
    """The analytic model of test_solver_host.py with every update on the device, eps evaluated in float64 from
    the device's x: the final x is the float64 host run's."""
    from ldm_amd import ops
    ab = ctx["ab"]
    times = SR.sample_times(99, 10)
    coef = ctx["ldm"].noise_scheduler.multistep_coefs(times).to(cuda)
    x_T = np.linspace(-2.0, 2.0, 4096)
    xd = torch.from_numpy(x_T).float().to(cuda)
    x0s = torch.empty((10, 4096), device=cuda)
    for i in range(10):
        eps = torch.from_numpy(SR.gauss_eps(ab, times[i], npy(xd))).float().to(cuda)
        ops.msolver_step_(xd, eps, coef[i].contiguous(), x0s[i], x0s[i - 1] if i else None)
    torch.cuda.synchronize()
    want, _, _ = SR.solve(ab, times, x_T, lambda xv, i: SR.gauss_eps(ab, times[i], xv))
    e = rel_err(npy(xd), want)
    print(f"gaussian model, 10 steps on the device: rel_err {e:.2e}")
    assert e <= UPD_TOL


# ---- dec1 with the fused update -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 16, 64), (1, 8, 8)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_step_dec1_msolver(ctx, cuda, B, H, W, dtype):
    from ldm_amd import _lib as L
    from ldm_amd import ops
    from ldm_amd.engine import UNetEngine
    u = ctx["ldm"].unet
    eng = UNetEngine(u, dtype=dtype)
    w = eng.weights(eng.shape(B, 32, H, W))
    dt = eng.step_dtype()
    coef = ctx["ldm"].noise_scheduler.multistep_coefs(SR.sample_times(99, 10))[4].contiguous()
    g = torch.Generator().manual_seed(31 + H)
    d2 = torch.randn(B, 64, H, W, generator=g)
    xs = torch.randn(B, 32, H, W, generator=g)
    prev = torch.randn(B, 32, H, W, generator=g)
    d2d = d2.permute(0, 2, 3, 1).contiguous().to(cuda)
    st = ops.stream_handle()
    for with_prev in (True, False):
        xsd = xs.permute(0, 2, 3, 1).contiguous().to(cuda)
        x0l = torch.full((B, 32, H, W), float("nan"), device=cuda)
        epl = torch.full_like(x0l, float("nan"))
        pd = prev.to(cuda) if with_prev else None
        L.call("ldm_step_dec1_msolver", B, H, W, d2d.data_ptr(), w.step_w[8], w.conv_b[8], coef.to(cuda).data_ptr(),
               xsd.data_ptr(), ops._p(pd), x0l.data_ptr(), epl.data_ptr(), dt, st)
        torch.cuda.synchronize()
        got = xsd.permute(0, 3, 1, 2).contiguous()
        c = table64(coef)
        if dtype == "fp32":
            eps = F.conv2d(d2.double(), u.dec1.weight.detach().double().cpu(), u.dec1.bias.detach().double().cpu(),
                           padding=1).numpy()
            assert rel_err(npy(epl), eps) <= UPD_TOL
        else:
            eps = npy(epl)       # the update is fp32 whatever the operands are: checked on the kernel's own eps
        xn, x0 = upd64(c, npy(xs), eps, npy(prev) if with_prev else None)
        e1, e2 = rel_err(npy(got), xn), rel_err(npy(x0l), x0)
        print(f"B {B} {H}x{W} {dtype} with_prev {with_prev}: x {e1:.2e}, x0 {e2:.2e}")
        assert e1 <= UPD_TOL and e2 <= UPD_TOL
        # bitwise the stand-alone kernel on that eps log
        x2 = xs.to(cuda).clone()
        x0b = torch.empty_like(x2)
        ops.msolver_step_(x2, epl, coef.to(cuda), x0b, pd)
        torch.cuda.synchronize()
        assert torch.equal(x2, got) and torch.equal(x0b, x0l)


# ---- the whole loop -------------------------------------------------------------------------------------------------
def run_loop(ctx, cuda, eng, z, s5, s6, times, split=1):
    B = z.shape[0]
    n = len(times) - 1
    coef = ctx["ldm"].noise_scheduler.multistep_coefs(torch.from_numpy(times)).to(cuda)
    t_table = torch.from_numpy(times[:-1]).view(n, 1).expand(n, B).contiguous().to(cuda)
    x = z.to(cuda).clone()
    x0l = torch.full((n,) + tuple(z.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    with torch.no_grad():
        eng.msolver_loop(x, s5.to(cuda), s6.to(cuda), t_table, coef, x0l, epl, split=split)
    torch.cuda.synchronize()
    return x, x0l, epl, coef


def check_loop(ctx, x, x0l, epl, coef, z, s5, s6, times, tag):
    """A float64 replay of the table recursion from the logged eps, then the lambda-form solver on the oracle UNet."""
    c = table64(coef)
    xv, prev = npy(z), None
    for i in range(len(times) - 1):
        xv, x0 = upd64(c[i], xv, npy(epl[i]), prev)
        e = rel_err(npy(x0l[i]), x0)
        assert e <= UPD_TOL, (tag, i, e)
        prev = x0
    e_replay = rel_err(npy(x), xv)
    want, _, _ = SR.sample(ctx["sd64"], ctx["ab"], times, npy(z), s5, s6)
    e_oracle = rel_err(npy(x), want)
    print(f"{tag}: replay {e_replay:.2e}, oracle {e_oracle:.2e}")
    assert e_replay <= UPD_TOL
    assert e_oracle <= PARITY_TOL


@pytest.fixture(scope="module")
def loop4(ctx, cuda):
    """engine.msolver_loop at B=2, 16x64, t_start 99, 4 steps on the default engine; shared, never modified."""
    z, s5, s6 = inputs(2, 16, 64, 11)
    times = SR.sample_times(99, 4)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    return (z, s5, s6, times) + run_loop(ctx, cuda, eng, z, s5, s6, times)


def test_loop_four_steps(ctx, loop4):
    z, s5, s6, times, x, x0l, epl, coef = loop4
    c = table64(coef)
    assert c[0, 4] == 0 and c[3, 4] == 0 and c[1, 4] != 0 and c[2, 4] != 0
    check_loop(ctx, x, x0l, epl, coef, z, s5, s6, times, "B2 16x64 4 steps")


@pytest.mark.parametrize("steps", [1, 2])
def test_loop_short(ctx, cuda, steps):
    z, s5, s6 = inputs(2, 16, 64, 12)
    times = SR.sample_times(99, steps)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    check_loop(ctx, *run_loop(ctx, cuda, eng, z, s5, s6, times), z, s5, s6, times, f"{steps} step(s)")


def test_loop_small_latent(ctx, cuda):
    z, s5, s6 = inputs(1, 8, 8, 13)                       # no bottleneck fold, 32-row dec1
    times = SR.sample_times(99, 4)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    check_loop(ctx, *run_loop(ctx, cuda, eng, z, s5, s6, times), z, s5, s6, times, "B1 8x8")


@pytest.mark.parametrize("kw", [dict(fold=False), dict(step=0)], ids=["unfolded", "folded-general"])
def test_loop_general_conv_epilogue(ctx, cuda, kw):
    """The loop on conv.hip's kernels (the literal UNet, and the folded one without step kernels)."""
    from ldm_amd.engine import UNetEngine
    z, s5, s6 = inputs(2, 16, 64, 14)
    times = SR.sample_times(99, 4)
    eng = UNetEngine(ctx["ldm"].unet, **kw)
    check_loop(ctx, *run_loop(ctx, cuda, eng, z, s5, s6, times), z, s5, s6, times, str(kw))


def test_per_layer_fallback(ctx, cuda):
    """A latent width the engine does not take: per-layer UNet + ops.msolver_step_."""
    M = ctx["M"]
    assert not M.UNetEngine.supports(4)
    torch.manual_seed(2)
    ldm4 = M.LDM(4, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm4.state_dict().items()}
    z, s5, s6 = inputs(2, 16, 16, 15, C=4)
    with torch.no_grad():
        x, logs = ldm4.style_conditioned_sample(z.to(cuda), {"s5": s5.to(cuda), "s6": s6.to(cuda)}, steps=3,
                                                t_start=99)
    torch.cuda.synchronize()
    times = SR.sample_times(99, 3)
    assert logs["timesteps"] == times[:-1].tolist()
    want, x0s, _ = SR.sample(sd64, ctx["ab"], times, npy(z), s5, s6)
    e = rel_err(npy(x), want)
    print(f"per-layer fallback: {e:.2e}")
    assert e <= PARITY_TOL
    assert rel_err(npy(logs["pred_x0"][1]), x0s[1]) <= PARITY_TOL


# ---- sub-batch chains and capture -----------------------------------------------------------------------------------
def test_split_and_capture(ctx, cuda):
    from ldm_amd.engine import GraphedDDIM
    z, s5, s6 = inputs(4, 16, 64, 16)
    times = SR.sample_times(99, 4)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x1, x0l1, epl1, coef = run_loop(ctx, cuda, eng, z, s5, s6, times)
    x2, x0l2, epl2, _ = run_loop(ctx, cuda, eng, z, s5, s6, times, split=2)
    e = max(rel_err(npy(x2), npy(x1)), rel_err(npy(x0l2), npy(x0l1)), rel_err(npy(epl2), npy(epl1)))
    print(f"split 2 against 1: {e:.2e}")
    assert e <= UPD_TOL
    t_table = torch.from_numpy(times[:-1]).view(4, 1).expand(4, 4).contiguous().to(cuda)
    with torch.no_grad():
        gd = GraphedDDIM(eng, z.to(cuda), s5.to(cuda), s6.to(cuda), t_table, coef, 0.0, logs=True, solver="msolver")
        a = gd.replay().clone()
        a0 = gd.x0_logs.clone()
        b = gd.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(a, x1) and torch.equal(a0, x0l1)
    assert torch.equal(b, x1) and torch.equal(gd.x0_logs, x0l1) and torch.equal(gd.eps_logs, epl1)


# ---- public methods -------------------------------------------------------------------------------------------------
def test_content_style_transfer_matches_the_composition(ctx, cuda):
    from oracle import ldm_torch_cpu as TC
    ldm, sd64, ab = ctx["ldm"], ctx["sd64"], ctx["ab"]
    g = torch.Generator().manual_seed(21)
    content = torch.rand(2, 1, 128, 128, generator=g)
    style = torch.rand(2, 1, 128, 128, generator=g)
    noise = torch.randn(2, 32, 16, 16, generator=g)
    with torch.no_grad():
        dec, zt_dec = ldm.content_style_transfer(content.to(cuda), style.to(cuda), t_start=99, steps=4,
                                                 noise=noise.to(cuda))
        torch.cuda.synchronize()
        z0 = TC.encoder(sd64, content.double())
        t = torch.full((2,), 99, dtype=torch.long)
        zt = TC.q_sample(torch.from_numpy(ab), z0, t, noise.double())
        emb = TC.style_encoder(sd64, style.double())
        times = SR.sample_times(99, 4)
        x, _, _ = SR.sample(sd64, ab, times, zt.numpy(), emb["s5"], emb["s6"])
        want = (TC.decoder(sd64, torch.from_numpy(x)) + 1) / 2
        want_zt = TC.decoder(sd64, zt)
    e1, e2 = rel_err(npy(dec), want.numpy()), rel_err(npy(zt_dec), want_zt.numpy())
    print(f"content_style_transfer: decoded {e1:.2e}, z_t decoded {e2:.2e}")
    assert e1 <= PARITY_TOL and e2 <= PARITY_TOL
    with torch.no_grad():       # the other solvers run, on the same grid
        for solver in ("dpmpp1", "ddim"):
            d, _ = ldm.content_style_transfer(content.to(cuda), style.to(cuda), t_start=99, steps=4, solver=solver,
                                              noise=noise.to(cuda))
            assert bool(torch.isfinite(d).all())
    with pytest.raises(ValueError):
        ldm.content_style_transfer(content.to(cuda), style.to(cuda), solver="heun")
    with pytest.raises(ValueError):
        ldm.content_style_transfer(content.to(cuda), style.to(cuda), t_start=5, steps=6)


def test_first_order_solver_is_ddim_eta0_on_the_same_grid(ctx, cuda):
    ldm = ctx["ldm"]
    z, s5, s6 = inputs(2, 16, 64, 22)
    emb = {"s5": s5.to(cuda), "s6": s6.to(cuda)}
    with torch.no_grad():
        a, _ = ldm.style_conditioned_sample(z.to(cuda), emb, steps=3, solver="dpmpp1", t_start=99)
        b, _ = ldm.style_conditioned_sample(z.to(cuda), emb, steps=3, solver="ddim", t_start=99)
    e = rel_err(npy(a), npy(b))
    print(f"dpmpp1 against ddim eta 0: {e:.2e}")
    assert e <= PARITY_TOL


# ---- the whole recording --------------------------------------------------------------------------------------------
def test_transfer_recording_with_a_solver(ctx, cuda):
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    from models.transfer import transfer_recording
    ldm = ctx["ldm"]
    content = torch.from_numpy(AR.test_signal(100 * 512)).float().to(cuda)     # 101 frames: two windows of 64 / 16
    style = torch.from_numpy(AR.test_signal(70 * 512, variant=1)).float().to(cuda)
    kw = dict(frames=64, overlap=16, n_iter=2, nnls_iters=2, seed=4)
    res = transfer_recording(ldm, content, style, num_timesteps=4, solver="dpmpp2m", **kw)
    assert res.N == 2
    x, ref = LF.mel_windows(A.melspectrogram(content), 64, 16)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 64, 0)
    noise = torch.randn((2, 32, 16, 8), generator=torch.Generator().manual_seed(4)).to(cuda)
    with torch.no_grad():
        want, _ = ldm.content_style_transfer(x, xs[:1].expand(2, -1, -1, -1).contiguous(), t_start=99, steps=4,
                                             solver="dpmpp2m", noise=noise)
    assert torch.equal(res.windows_out, want)
    assert torch.equal(res.mel_power, LF.stitch_windows(want, ref, 16, 101))
    assert torch.equal(res.audio, A.mel_to_audio(res.mel_power, seed=4, length=100 * 512, n_iter=2, nnls_iters=2))
    # solver=None is today's call, bit for bit
    res0 = transfer_recording(ldm, content, style, num_timesteps=3, **kw)
    with torch.no_grad():
        want0, _ = ldm.content_style_transfer_wrapper(x, xs[:1].expand(2, -1, -1, -1).contiguous(), num_timesteps=3,
                                                      eta=0.0, noise=noise)
    assert torch.equal(res0.windows_out, want0)
    assert torch.equal(res0.audio, A.mel_to_audio(LF.stitch_windows(want0, ref, 16, 101), seed=4, length=100 * 512,
                                                  n_iter=2, nnls_iters=2))
    with pytest.raises(ValueError):
        transfer_recording(ldm, content, style, num_timesteps=4, t_start=50, **kw)
