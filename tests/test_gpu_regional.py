"""GPU: the regional keep (x_next = (1 - w) x_update + w (a z0 + b n0) behind the fused update) from the stand-alone
kernel up to transfer_recording, against the float64 yardstick tests/regional_ref.py and the oracle's UNet.

Bars.  w = 0 leaves the update's value, so the keep loop is held bitwise to the loop without it; w = 1 leaves
a z0 + b n0, held bitwise to the same fp32 operations in torch.  Against float64 a mixed mask may cost at most twice
the error of the corresponding loop without the keep on the same inputs, measured in the same test (the two loops'
trajectories differ), and never more than 1e-4, the loops' existing bar."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR        # noqa: E402
import guidance_ref as GR     # noqa: E402
import regional_ref as RR     # noqa: E402
import solver_ref as SR       # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN_TOL = 1e-4
SOLVERS = [("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m", 0.0)]
SOLVER_IDS = ["ddim-eta0", "ddim-eta1", "dpmpp2m"]
STEPS = 4
# tests/test_gpu_guidance.py's LOOPS: the step kernels at the canonical latent and at an odd batch on a small one,
# conv.hip's loops (folded without step kernels, unfolded)
LOOPS = [("default", 2, 16, 64), ("default", 3, 8, 16), ("folded-general", 2, 16, 16), ("unfolded", 2, 16, 16)]
LOOP_IDS = ["step-2x16x64", "step-3x8x16", "folded-general-2x16x16", "unfolded-2x16x16"]


def npy(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def ctx(cuda):
    """The model (never modified), its float64 state dict and schedule."""
    import models.model as M
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm.state_dict().items()}
    return dict(M=M, ldm=ldm, sd64=sd64, ab=SR.alpha_bar(ldm.num_timesteps), times=SR.sample_times(99, STEPS), cache={})


def inputs(ctx, B, H, W, seed, C=32):
    """z0, n0, x = q_sample(z0, 99, n0) in fp32, and two distinct style-map pairs."""
    g = torch.Generator().manual_seed(seed)
    z0, n0 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    maps = [torch.rand(B, 256, H // 4, W // 4, generator=g), torch.rand(B, 512, H // 8, W // 8, generator=g),
            torch.rand(B, 256, H // 4, W // 4, generator=g), torch.rand(B, 512, H // 8, W // 8, generator=g)]
    ab = float(ctx["ab"][99])
    x = float(np.float32(np.sqrt(ab))) * z0 + float(np.float32(np.sqrt(1 - ab))) * n0
    return x, z0, n0, (maps[0], maps[1]), (maps[2], maps[3])


def mask(B, H, W, variant=0):
    """A keep mask that differs per sample: a column band that is not aligned to a wave's 16 columns, a row band, a
    soft value, and where B allows an all-one and an all-zero sample."""
    w = torch.zeros(B, H, W)
    c1 = min(22, W - 2)
    w[0, :, 5:c1 + 1] = 1.0                      # columns 5 .. 22 (5 .. W - 2 on a narrow latent)
    w[0, H - 3:, :4] = 0.25
    w[1 % B, 3:6, :] = 1.0                       # rows 3 .. 5
    w[1 % B, 0, 1::2] = 0.25
    if B >= 3:
        w[2] = 1.0
    if B >= 4:
        w[3] = 0.0
    if variant:                                  # another mask of the same kind (set_keep)
        w = torch.flip(w, dims=(0, 2)).contiguous()
    return w


def coef_tables(ctx, cuda, solver, B):
    tt = torch.from_numpy(ctx["times"])
    fd = ctx["ldm"].noise_scheduler
    coef = (fd.multistep_coefs(tt) if solver != "ddim" else fd.reverse_coefs(tt)).to(cuda)
    t_table = tt[:-1].view(STEPS, 1).expand(STEPS, B).contiguous().to(cuda)
    return tt, fd, coef, t_table


def run(ctx, cuda, eng, solver, eta, x_in, tgt, keep=None, base=None, scale=1.0, split=1, exact_last=True):
    """One loop on the engine.  keep = (z0, n0, w) or None.  Returns (x, x0_logs, eps_logs)."""
    B = x_in.shape[0]
    tt, fd, coef, t_table = coef_tables(ctx, cuda, solver, B)
    x = x_in.to(cuda).clone()
    x0l = torch.full((STEPS,) + tuple(x_in.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    kw = dict(split=split)
    if base is not None:
        kw.update(base=(base[0].to(cuda), base[1].to(cuda), None, None), guidance_scale=scale)
    if keep is not None:
        kw.update(keep=dict(z0=keep[0].to(cuda), n0=keep[1].to(cuda), w=keep[2].to(cuda), coefs=fd.keep_coefs(tt, exact_last)))
    with torch.no_grad():
        if solver == "ddim":
            eng.ddim_loop(x, tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, x0l, epl, **kw)
        else:
            eng.msolver_loop(x, tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, x0l, epl, **kw)
    torch.cuda.synchronize()
    return x, x0l, epl


def engine(ctx, kind):
    from ldm_amd.engine import UNetEngine
    if kind == "default":
        return ctx["M"].engine_for(ctx["ldm"].unet)
    return UNetEngine(ctx["ldm"].unet, **{"unfolded": dict(fold=False), "folded-general": dict(step=0)}[kind])


def errs3(got, want):
    """Relative errors of the final x, the x0 logs and the eps logs against float64."""
    x, x0l, epl = got
    wx, x0s, epss = want
    return rel_err(npy(x), wx), rel_err(npy(x0l), np.stack(x0s)), rel_err(npy(epl), np.stack(epss))


# ---- 1. w = 0: bitwise the loop without the keep ---------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_zero_weight_is_the_plain_loop_bitwise(ctx, cuda, kind, B, H, W, solver, eta):
    eng = engine(ctx, kind)
    x, z0, n0, tgt, base = inputs(ctx, B, H, W, 100 + H + W)
    zero = torch.zeros(B, H, W)
    for guide in ({}, dict(base=base, scale=3.0)):
        p = run(ctx, cuda, eng, solver, eta, x, tgt, **guide)
        k = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, zero), **guide)
        for name, u, v in zip(("x", "x0 logs", "eps logs"), p, k):
            assert torch.equal(u, v), (name, "guided" if guide else "plain")


# ---- 2. w = 1: the content's trajectory, whatever the denoiser says --------------------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_full_weight_ends_on_the_contents_trajectory_bitwise(ctx, cuda, kind, B, H, W, solver, eta):
    eng = engine(ctx, kind)
    x, z0, n0, tgt, base = inputs(ctx, B, H, W, 150 + H + W)
    one = torch.ones(B, H, W)
    tt = torch.from_numpy(ctx["times"])
    a, b = ctx["ldm"].noise_scheduler.keep_coefs(tt, exact_last=False)[-1]
    known = a * z0 + b * n0                                   # keep_blend's op sequence in fp32, one rounding each
    k, _, _ = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, one), exact_last=False)
    assert torch.equal(k.cpu(), known)
    k, _, _ = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, one))
    assert torch.equal(k.cpu(), z0)
    k, _, _ = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, one), base=base, scale=3.0)
    assert torch.equal(k.cpu(), z0)


# ---- 3. a mixed mask against float64 ---------------------------------------------------------------------------------
def plain_result(ctx, cuda, kind, B, H, W, solver, eta):
    """The plain loop's errors against float64 (final x, x0 logs, eps logs) on the inputs of test 3, computed once per
    configuration, shared, never modified."""
    key = (kind, B, H, W, solver, eta)
    if key not in ctx["cache"]:
        x, z0, n0, tgt, _ = inputs(ctx, B, H, W, 200 + H + W)
        got = run(ctx, cuda, engine(ctx, kind), solver, eta, x, tgt)
        ctx["cache"][key] = errs3(got, GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(x), tgt, solver, eta))
    return ctx["cache"][key]


@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_mixed_mask_against_float64(ctx, cuda, kind, B, H, W, solver, eta):
    """x and both logs, each held to min(2 e_plain, 1e-4) of the same quantity.  Measured values: DESIGN.md 7g."""
    e_plain = plain_result(ctx, cuda, kind, B, H, W, solver, eta)
    x, z0, n0, tgt, _ = inputs(ctx, B, H, W, 200 + H + W)
    w = mask(B, H, W)
    got = run(ctx, cuda, engine(ctx, kind), solver, eta, x, tgt, keep=(z0, n0, w))
    e = errs3(got, RR.sample(ctx["sd64"], ctx["ab"], ctx["times"], npy(x), tgt, npy(z0), npy(n0), npy(w), solver, eta))
    print(f"{kind} B{B} {H}x{W} {solver} eta {eta}: keep x {e[0]:.2e} x0 {e[1]:.2e} eps {e[2]:.2e}; plain x {e_plain[0]:.2e} "
          f"x0 {e_plain[1]:.2e} eps {e_plain[2]:.2e}")
    for q in range(3):
        assert e[q] <= min(2.0 * e_plain[q], PLAIN_TOL), ("x", "x0 logs", "eps logs")[q]


# ---- 4. composition with the guidance and with a mix -----------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_guided_keep_against_float64(ctx, cuda, kind, B, H, W, solver, eta):
    """Per-sample strengths up to 3; the bar is the guided loop's own error without the keep on the same inputs."""
    x, z0, n0, tgt, base = inputs(ctx, B, H, W, 300 + H + W)
    sv = np.array([3.0, 0.5, -1.25][:B])
    scale = torch.from_numpy(sv).float()
    w = mask(B, H, W)
    eng = engine(ctx, kind)
    args = (ctx["sd64"], ctx["ab"], ctx["times"], npy(x))
    e_g = errs3(run(ctx, cuda, eng, solver, eta, x, tgt, base=base, scale=scale), GR.sample(*args, tgt, base, sv, solver, eta))
    got = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, w), base=base, scale=scale)
    e = errs3(got, RR.sample(*args, tgt, npy(z0), npy(n0), npy(w), solver, eta, base=base, s=sv))
    print(f"{kind} B{B} {H}x{W} {solver} eta {eta} guided: keep x {e[0]:.2e} x0 {e[1]:.2e} eps {e[2]:.2e}; guided alone "
          f"x {e_g[0]:.2e} x0 {e_g[1]:.2e} eps {e_g[2]:.2e}")
    # both halves' copies of the state got the blended value: the next step's base half started from it
    for q in range(3):
        assert e[q] <= min(2.0 * e_g[q], PLAIN_TOL), ("x", "x0 logs", "eps logs")[q]


def test_mix_with_keep_against_float64(ctx, cuda):
    import stylemix_ref as MR
    ldm = ctx["ldm"]
    B, H, W = 2, 16, 16
    x, z0, n0, _, _ = inputs(ctx, B, H, W, 401)
    g = torch.Generator().manual_seed(402)
    specs = torch.rand(B, 2, 1, 128, 128, generator=g).to(cuda)
    w = mask(B, H, W)
    with torch.no_grad():
        emb = ldm.encode_styles(specs, [0.25, 0.75])
        assert emb["refs"] == 2
        xp, lp = ldm.style_conditioned_sample(x.to(cuda), emb, steps=STEPS, t_start=99)
        xk, lk = ldm.style_conditioned_sample(x.to(cuda), emb, steps=STEPS, t_start=99, keep=w.to(cuda), z0=z0.to(cuda),
                                              noise=n0.to(cuda))
    torch.cuda.synchronize()
    L2, L1 = (H // 4) * (W // 4), (H // 8) * (W // 8)
    tgt = (emb["s5"].cpu(), emb["s6"].cpu(), MR.key_weights([0.25, 0.75], B, 2, L2), MR.key_weights([0.25, 0.75], B, 2, L1))
    args = (ctx["sd64"], ctx["ab"], ctx["times"], npy(x))
    stack = lambda xv, logs: (xv, torch.stack(logs["pred_x0"]), torch.stack(logs["noise_pred"]))      # noqa: E731
    e_p = errs3(stack(xp, lp), GR.sample_plain(*args, tgt))
    e = errs3(stack(xk, lk), RR.sample(*args, tgt, npy(z0), npy(n0), npy(w)))
    print(f"mix R 2 (0.25, 0.75) with keep: x {e[0]:.2e} x0 {e[1]:.2e} eps {e[2]:.2e}; the mix alone x {e_p[0]:.2e} "
          f"x0 {e_p[1]:.2e} eps {e_p[2]:.2e}")
    for q in range(3):
        assert e[q] <= min(2.0 * e_p[q], PLAIN_TOL), ("x", "x0 logs", "eps logs")[q]


# ---- 5. 16-bit operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16_bit_operands(ctx, cuda, dt):
    """Inside torch.autocast at the canonical latent: at most twice the single-style 16-bit loop's error against
    float64 on the same inputs (the blend is fp32 and adds no 16-bit rounding).  Measured values: DESIGN.md 7g."""
    from ldm_amd.engine import UNetEngine
    x, z0, n0, tgt, _ = inputs(ctx, 2, 16, 64, 501)
    w = mask(2, 16, 64)
    eng = UNetEngine(ctx["ldm"].unet)
    with torch.autocast("cuda", dtype=dt):
        assert eng.step_dtype() == (1 if dt == torch.float16 else 2)
        xk, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, x, tgt, keep=(z0, n0, w))
        xp, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, x, tgt)
    args = (ctx["sd64"], ctx["ab"], ctx["times"], npy(x))
    wk, _, _ = RR.sample(*args, tgt, npy(z0), npy(n0), npy(w))
    wp, _, _ = GR.sample_plain(*args, tgt)
    e, e_p = rel_err(npy(xk), wk), rel_err(npy(xp), wp)
    print(f"{dt}: keep {e:.3e}; single style {e_p:.3e}")
    assert e <= 2.0 * e_p


# ---- 6. capture, set_keep, split -------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_capture_and_set_keep(ctx, cuda, solver, eta, guided):
    from ldm_amd.engine import GraphedDDIM
    B = 4
    x, z0, n0, tgt, base = inputs(ctx, B, 16, 64, 601)
    eng = engine(ctx, "default")
    w_a, w_b = mask(B, 16, 64), mask(B, 16, 64, variant=1)
    s = torch.tensor([3.0, 0.5, -1.25, 2.0])
    guide = dict(base=base, scale=s) if guided else {}
    a = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, w_a), **guide)
    b = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, w_b), **guide)
    assert not torch.equal(a[0], b[0])
    tt, fd, coef, t_table = coef_tables(ctx, cuda, solver, B)
    gkw = dict(base=(base[0].to(cuda), base[1].to(cuda), None, None), guidance_scale=s) if guided else {}
    with torch.no_grad():
        gd = GraphedDDIM(eng, x.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, logs=True,
                         solver="msolver" if solver != "ddim" else "ddim",
                         keep=(z0.to(cuda), n0.to(cuda), w_a.to(cuda), fd.keep_coefs(tt)), **gkw)
        r = gd.replay().clone()
        torch.cuda.synchronize()
        assert torch.equal(r, a[0]) and torch.equal(gd.x0_logs, a[1]) and torch.equal(gd.eps_logs, a[2])
        gd.set_keep(w_b)
        r = gd.replay().clone()
        torch.cuda.synchronize()
        assert torch.equal(r, b[0]) and torch.equal(gd.x0_logs, b[1]) and torch.equal(gd.eps_logs, b[2])
        with pytest.raises(ValueError):
            gd.set_keep(w_b + 1)
    if guided:      # the guided form's chains run the whole batch's plans: split = 2 is split = 1 bit for bit
        c = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, w_a), split=2, **guide)
        for name, u, v in zip(("x", "x0 logs", "eps logs"), a, c):
            assert torch.equal(u, v), name
        with torch.no_grad():
            gd = GraphedDDIM(eng, x.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, logs=True, split=2,
                             solver="msolver" if solver != "ddim" else "ddim",
                             keep=(z0.to(cuda), n0.to(cuda), w_a.to(cuda), fd.keep_coefs(tt)), **gkw)
            r = gd.replay().clone()
        torch.cuda.synchronize()
        assert torch.equal(r, a[0]) and torch.equal(gd.x0_logs, a[1]) and torch.equal(gd.eps_logs, a[2])
    else:           # the plain loop's chains are "the same up to fp32 summation order": the slices must be the right ones
        c = run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, w_a), split=2)
        assert rel_err(npy(c[0]), npy(a[0])) <= 1e-5


# ---- 7. the stand-alone kernel and the per-layer fallback ------------------------------------------------------------
def test_keep_blend_kernel(cuda):
    from ldm_amd import ops
    g = torch.Generator().manual_seed(701)
    xu, z0, n0 = (torch.randn(3, 5, 7, 9, generator=g) for _ in range(3))
    w = torch.rand(3, 7, 9, generator=g)
    w[0], w[1, :3] = 0.0, 1.0
    coef = torch.tensor([0.8125, 0.59375]) + torch.tensor([1e-3, 2e-3])
    got = ops.keep_blend_(xu.to(cuda).clone(), z0.to(cuda), n0.to(cuda), w.to(cuda), coef.to(cuda)).cpu()
    torch.cuda.synchronize()
    wv = w[:, None]
    known = coef[0] * z0 + coef[1] * n0
    assert torch.equal(got, (1.0 - wv) * xu + wv * known)      # the definition's op sequence, one rounding each
    assert torch.equal(got[0], xu[0]) and torch.equal(got[1, :, :3], known[1, :, :3])
    e = rel_err(npy(got), RR.keep_blend(npy(xu), npy(z0), npy(n0), npy(w), float(coef[0]), float(coef[1])))
    print(f"ldm_keep_blend: {e:.2e}")
    assert e <= 1e-6
    with pytest.raises(ValueError):
        ops.keep_blend_(xu.to(cuda), z0.to(cuda), n0.to(cuda), w[:2].to(cuda), coef.to(cuda))


@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
def test_per_layer_fallback(ctx, cuda, solver, eta):
    """A latent width the engine does not take: per-layer UNet calls, the update kernel, then ldm_keep_blend."""
    M = ctx["M"]
    assert not M.UNetEngine.supports(4)
    torch.manual_seed(2)
    ldm4 = M.LDM(4, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm4.state_dict().items()}
    x, z0, n0, tgt, _ = inputs(ctx, 2, 16, 16, 702, C=4)
    w = mask(2, 16, 16)
    emb = {"s5": tgt[0].to(cuda), "s6": tgt[1].to(cuda)}
    with torch.no_grad():
        xp, _ = ldm4.style_conditioned_sample(x.to(cuda), emb, steps=STEPS, t_start=99, solver=solver, eta=eta)
        xk, logs = ldm4.style_conditioned_sample(x.to(cuda), emb, steps=STEPS, t_start=99, solver=solver, eta=eta,
                                                 keep=w.to(cuda), z0=z0.to(cuda), noise=n0.to(cuda))
    torch.cuda.synchronize()
    args = (sd64, ctx["ab"], ctx["times"], npy(x))
    wp, _, _ = GR.sample_plain(*args, tgt, solver, eta)
    wk, x0s, _ = RR.sample(*args, tgt, npy(z0), npy(n0), npy(w), solver, eta)
    e_p, e = rel_err(npy(xp), wp), rel_err(npy(xk), wk)
    print(f"per-layer fallback {solver} eta {eta}: keep {e:.2e}; plain {e_p:.2e}")
    assert e <= min(2.0 * e_p, PLAIN_TOL) and rel_err(npy(logs["pred_x0"][1]), x0s[1]) <= PLAIN_TOL


# ---- 8. / 9. the public methods --------------------------------------------------------------------------------------
def test_content_style_transfer_and_transfer_recording(ctx, cuda):
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    from models.transfer import HOP, transfer_recording
    ldm = ctx["ldm"]
    content = torch.from_numpy(AR.test_signal(900 * 512)).float().to(cuda)      # 901 frames: two windows of 512 / 64
    style = torch.from_numpy(AR.test_signal(520 * 512, variant=1)).float().to(cuda)
    kw = dict(frames=512, overlap=64, n_iter=2, nnls_iters=2, seed=4, num_timesteps=STEPS, solver="dpmpp2m")
    x, ref = LF.mel_windows(A.melspectrogram(content), 512, 64)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 512, 0)
    assert x.shape[0] == 2 and HOP == 512
    st2 = xs[:1].expand(2, -1, -1, -1).contiguous()
    noise = torch.randn((2, 32, 16, 64), generator=torch.Generator().manual_seed(4)).to(cuda)
    ckw = dict(t_start=99, steps=STEPS, solver="dpmpp2m", noise=noise)
    # frames 100 .. 599 of the recording: the tail of window 0 and, past the seam, the head of window 1
    sr = 22050
    full = LF.keep_mask(901, 128, sr, times=[(100 * 512 / sr, 599 * 512 / sr + 1e-6)], feather=16)
    M = LF.mask_windows(full, 512, 64).to(cuda)
    assert tuple(M.shape) == (2, 1, 128, 512) and float(M[0, 0, 0, 130]) == 1.0 and float(M[0, 0, 0, 99]) == 0.0
    with torch.no_grad():
        plain, _ = ldm.content_style_transfer(x, st2, **ckw)
        comp, _ = ldm.content_style_transfer(x, st2, keep=M, **ckw)
        raw, _ = ldm.content_style_transfer(x, st2, keep=M, composite=False, **ckw)
        lat, _ = ldm.content_style_transfer(x, st2, keep=ldm.latent_keep(M), **ckw)
        none, _ = ldm.content_style_transfer(x, st2, keep=None, **ckw)
    one, free = (M == 1).expand_as(x), (M == 0).expand_as(x)
    assert torch.equal(none, plain)                                        # without the argument: the call it always was
    assert torch.equal(comp[one], x[one])                                  # the kept region comes back as it went in
    assert torch.equal(comp[free], raw[free]) and torch.equal(lat, raw)    # composite touches only M > 0; latent masks never
    assert not torch.equal(raw[one], x[one]) and not torch.equal(raw, plain)
    assert bool(torch.isfinite(comp).all()) and bool(torch.isfinite(raw).all())
    # (printed only, the weights are untrained: how far the kept region of window 0 decodes from the content)
    assert bool((M[0, :, :, 160:400] == 1).all())
    d_keep = (raw[0, :, :, 160:400] - x[0, :, :, 160:400]).abs().mean()
    d_plain = (plain[0, :, :, 160:400] - x[0, :, :, 160:400]).abs().mean()
    print(f"decoded kept region against the content: keep {float(d_keep):.3e}, no keep {float(d_plain):.3e}")
    # the whole recording, with and without guidance
    res = transfer_recording(ldm, content, style, keep=full, **kw)
    assert res.N == 2 and torch.equal(res.windows_out, comp)
    res_raw = transfer_recording(ldm, content, style, keep=full, composite=False, **kw)
    assert torch.equal(res_raw.windows_out, raw)
    res_g = transfer_recording(ldm, content, style, keep=full, guidance_scale=2.0, **kw)
    assert bool(torch.isfinite(res_g.windows_out).all()) and not torch.equal(res_g.windows_out, comp)
    assert torch.equal(res_g.windows_out[one], x[one])
    # inside the kept span, away from the feather, the stitched mel is the content's stitched mel
    mel_c = LF.stitch_windows(x, ref, 64, 901)
    span = slice(100 + 16, 600 - 16)
    for r in (res, res_g):
        assert rel_err(npy(r.mel_power[:, span]), npy(mel_c[:, span])) <= 1e-6
    assert rel_err(npy(res.mel_power[:, :90]), npy(mel_c[:, :90])) > 1e-3      # and is something else outside it
    res0 = transfer_recording(ldm, content, style, **kw)                       # without the new arguments
    assert torch.equal(res0.windows_out, plain)
    with pytest.raises(ValueError, match="solver"):
        transfer_recording(ldm, content, style, keep=full, **dict(kw, solver=None))


# ---- 10. errors of the C entry points --------------------------------------------------------------------------------
def test_c_abi_errors(ctx, cuda):
    import ctypes
    from ldm_amd import _lib as L
    from ldm_amd import ops
    eng = engine(ctx, "default")
    B, H, W = 2, 8, 16
    xin, z0, n0, tgt, base = inputs(ctx, B, H, W, 901)
    shape = eng.shape(B, 32, H, W)
    w = eng.weights(shape)
    ws = eng.workspace(shape, cuda, STEPS, keep=True)

    def size(**fields):
        return int(L.load().ldm_sample_workspace_floats(ctypes.byref(shape), ctypes.byref(w), ctypes.byref(L.SampleArgs(**fields))))

    n_plain, n_keep = size(nsteps=STEPS), size(nsteps=STEPS, z0=1, n0=1, keep=1, keep_coef=1)
    assert n_keep == n_plain + 2 * B * 32 * H * W + B * H * W + 2 * STEPS and ws.numel() >= n_keep
    assert size(nsteps=-1, z0=1, n0=1, keep=1, keep_coef=1) < 0
    x = xin.to(cuda).clone()
    d = [t.to(cuda) for t in tgt]
    tt, fd, c8, t_table = coef_tables(ctx, cuda, "dpmpp2m", B)
    c4 = fd.reverse_coefs(tt).to(cuda)
    kops = [z0.to(cuda), n0.to(cuda), mask(B, H, W).to(cuda), fd.keep_coefs(tt).to(cuda)]
    x0l = torch.empty((STEPS,) + tuple(xin.shape), device=cuda)

    def call(solver, kp, coef, wsp):
        a = L.SampleArgs(solver=L.SOLVER[solver], nsteps=STEPS, eta=0.0, x=x.data_ptr(), s5=d[0].data_ptr(),
                         s6=d[1].data_ptr(), z0=kp[0], n0=kp[1], keep=kp[2], keep_coef=kp[3], t_table=t_table.data_ptr(),
                         coef_table=coef.data_ptr(), x0_logs=x0l.data_ptr(), workspace=wsp, stream=ops.stream_handle())
        L.call("ldm_sample", ctypes.byref(shape), ctypes.byref(w), ctypes.byref(a))

    forms = (("ddim", c4), ("msolver", c8))
    for name, coef in forms:
        for missing in range(4):
            kp = [None if j == missing else t.data_ptr() for j, t in enumerate(kops)]
            with pytest.raises(L.LDMError, match="keep"):
                call(name, kp, coef, ws.data_ptr())
    with pytest.raises(L.LDMError):
        L.call("ldm_keep_blend", x.data_ptr(), None, kops[1].data_ptr(), kops[2].data_ptr(), kops[3].data_ptr(), B, 32, H * W,
               ops.stream_handle())
    # a workspace sized for the plain loop, as an allocation of its own (the entry asks the runtime for the extent
    # of the allocation that holds the pointer; torch's caching allocator would hand out part of a larger one)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], ctypes.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [ctypes.c_void_p], ctypes.c_int
    short = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(short), n_plain * 4) == 0
    try:
        for name, coef in forms:
            with pytest.raises(L.LDMError, match="workspace"):
                call(name, [t.data_ptr() for t in kops], coef, short.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipFree(short) == 0
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), xin)          # nothing ran
    # with a NULL keep the loop is the plain one; the good call works afterwards
    call("ddim", [None] * 4, c4, ws.data_ptr())
    torch.cuda.synchronize()
    p, _, _ = run(ctx, cuda, eng, "ddim", 0.0, xin, tgt)
    assert torch.equal(x, p)
    x.copy_(xin)
    call("ddim", [t.data_ptr() for t in kops], c4, ws.data_ptr())
    torch.cuda.synchronize()
    k, _, _ = run(ctx, cuda, eng, "ddim", 0.0, xin, tgt, keep=(z0, n0, mask(B, H, W)))
    assert torch.equal(x, k) and not torch.equal(x, p)
