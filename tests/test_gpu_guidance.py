"""GPU: style guidance (eps = e_b + s (e_t - e_b) in front of the fused update) from the stand-alone kernel up to
transfer_recording, against the float64 yardstick tests/guidance_ref.py and the oracle's UNet.

Bars.  With target == base the difference is exactly zero, so the guided loop is held bitwise to the first half of the
plain loop at twice the batch.  Against float64 the guided error may be at most (1 + 2|s|) times a plain loop's (the
worst-case amplification of e_b + s (e_t - e_b)): <= 2 (1 + 2|s|) max(e_t, e_b) with the plain loops' errors measured
in the same test, and <= (1 + 2|s|) 1e-4, 1e-4 being the loops' existing bar.  s = 0 / s = 1 against the plain base /
target loop: 1e-5, the fold tests' bar."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR        # noqa: E402
import guidance_ref as GR     # noqa: E402
import solver_ref as SR       # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN_TOL, FOLD_TOL = 1e-4, 1e-5
SOLVERS = [("ddim", 0.0), ("ddim", 1.0), ("dpmpp2m", 0.0)]
SOLVER_IDS = ["ddim-eta0", "ddim-eta1", "dpmpp2m"]
STEPS = 4


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


def inputs(B, H, W, seed, C=32):
    """z and two distinct style-map pairs (target, base)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g)
    maps = [torch.rand(B, 256, H // 4, W // 4, generator=g), torch.rand(B, 512, H // 8, W // 8, generator=g),
            torch.rand(B, 256, H // 4, W // 4, generator=g), torch.rand(B, 512, H // 8, W // 8, generator=g)]
    return z, (maps[0], maps[1]), (maps[2], maps[3])


def run(ctx, cuda, eng, solver, eta, z, tgt, base=None, scale=1.0, split=1, kb=(None, None), kb_base=(None, None)):
    """One loop on the engine: the plain one (base None) or the guided one.  Returns (x, x0_logs, eps_logs)."""
    times = ctx["times"]
    B, n = z.shape[0], len(times) - 1
    fd = ctx["ldm"].noise_scheduler
    tt = torch.from_numpy(times)
    coef = (fd.multistep_coefs(tt) if solver != "ddim" else fd.reverse_coefs(tt)).to(cuda)
    t_table = tt[:-1].view(n, 1).expand(n, B).contiguous().to(cuda)
    x = z.to(cuda).clone()
    x0l = torch.full((n,) + tuple(z.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    kw = dict(split=split, key_bias5=kb[0], key_bias6=kb[1])
    if base is not None:
        kw.update(base=(base[0].to(cuda), base[1].to(cuda), kb_base[0], kb_base[1]), guidance_scale=scale)
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


# the step kernels at the canonical latent (variant-3 windowed / plane forms, the value fold at internal batch 4) and
# at an odd batch on a small latent (the non-window forms); conv.hip's loops (folded without step kernels, unfolded)
LOOPS = [("default", 2, 16, 64), ("default", 3, 8, 16), ("folded-general", 2, 16, 16), ("unfolded", 2, 16, 16)]
LOOP_IDS = ["step-2x16x64", "step-3x8x16", "folded-general-2x16x16", "unfolded-2x16x16"]


# ---- 1. target == base: bitwise the plain loop at twice the batch ----------------------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_same_target_and_base_is_the_plain_loop_at_twice_the_batch_bitwise(ctx, cuda, kind, B, H, W, solver, eta):
    eng = engine(ctx, kind)
    z, tgt, _ = inputs(B, H, W, 100 + H + W)
    two = lambda t: torch.cat([t, t])      # noqa: E731
    px, px0, pep = run(ctx, cuda, eng, solver, eta, two(z), (two(tgt[0]), two(tgt[1])))
    assert torch.equal(px[:B], px[B:])
    for scale in (3.7, torch.tensor([3.7, -1.25, 0.5][:B])):
        x, x0l, epl = run(ctx, cuda, eng, solver, eta, z, tgt, base=tgt, scale=scale)
        assert torch.equal(x, px[:B]), "x"
        assert torch.equal(x0l, px0[:, :B]), "x0 logs"
        assert torch.equal(epl, pep[:, :B]), "eps logs"


# ---- 2. against float64 ----------------------------------------------------------------------------------------------
def errs3(x, x0l, epl, want, x0s, epss):
    """Relative errors of the final x, the x0 logs and the eps logs against float64."""
    return rel_err(npy(x), want), rel_err(npy(x0l), np.stack(x0s)), rel_err(npy(epl), np.stack(epss))


def plain_errors(ctx, cuda, kind, B, H, W, solver, eta):
    """The plain loop's relative errors against float64 (final x, x0 logs, eps logs) on the target and on the base
    maps, and the two device results (computed once per configuration, shared, never modified)."""
    key = (kind, B, H, W, solver, eta)
    if key not in ctx["cache"]:
        eng = engine(ctx, kind)
        z, tgt, base = inputs(B, H, W, 200 + H + W)
        out = []
        for maps in (tgt, base):
            x, x0l, epl = run(ctx, cuda, eng, solver, eta, z, maps)
            out.append((errs3(x, x0l, epl, *GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), maps, solver, eta)), x))
        ctx["cache"][key] = out
    return ctx["cache"][key]


def bars(s, e_t, e_b):
    smax = float(np.max(np.abs(np.asarray(s, dtype=np.float64))))
    amp = 1.0 + 2.0 * smax
    return min(2.0 * amp * max(e_t, e_b), amp * PLAIN_TOL)


SCALES = [0.0, 0.5, 3.0, "per-sample"]


@pytest.mark.parametrize("s", SCALES, ids=[str(s) for s in SCALES])
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_guided_loop_against_float64(ctx, cuda, kind, B, H, W, solver, eta, s):
    """The final x, and the guided x0 / eps logs each against the plain loops' error of the same quantity.
    Measured on an MI355X: see the table there."""
    (e_t, _), (e_b, _) = plain_errors(ctx, cuda, kind, B, H, W, solver, eta)
    z, tgt, base = inputs(B, H, W, 200 + H + W)
    sv = np.array([0.0, 3.0, 0.5][:B] if B == 3 else [3.0, 0.5]) if s == "per-sample" else s
    scale = torch.from_numpy(sv).float() if s == "per-sample" else s
    x, x0l, epl = run(ctx, cuda, engine(ctx, kind), solver, eta, z, tgt, base=base, scale=scale)
    e = errs3(x, x0l, epl, *GR.sample(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), tgt, base, sv, solver, eta))
    bar = [bars(sv, e_t[q], e_b[q]) for q in range(3)]
    print(f"{kind} B{B} {H}x{W} {solver} eta {eta} s {s}: x {e[0]:.2e} x0 {e[1]:.2e} eps {e[2]:.2e}; plain (x, x0, eps) "
          f"e_t {e_t[0]:.2e} {e_t[1]:.2e} {e_t[2]:.2e} e_b {e_b[0]:.2e} {e_b[1]:.2e} {e_b[2]:.2e}; bar x {bar[0]:.2e}")
    for q in range(3):
        assert e[q] <= bar[q], ("x", "x0 logs", "eps logs")[q]


# ---- 3. s = 0 is the plain base loop, s = 1 with a base the plain target loop ----------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_scale_zero_and_one_are_the_plain_loops(ctx, cuda, kind, B, H, W, solver, eta):
    (_, x_t), (_, x_b) = plain_errors(ctx, cuda, kind, B, H, W, solver, eta)
    z, tgt, base = inputs(B, H, W, 200 + H + W)
    eng = engine(ctx, kind)
    g0, _, _ = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=0.0)
    g1, _, _ = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=1.0)
    e0, e1 = rel_err(npy(g0), npy(x_b)), rel_err(npy(g1), npy(x_t))
    print(f"{kind} B{B} {H}x{W} {solver} eta {eta}: s=0 vs base loop {e0:.2e}, s=1 vs target loop {e1:.2e}")
    assert e0 <= FOLD_TOL and e1 <= FOLD_TOL


# ---- 4. 16-bit operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16_bit_operands(ctx, cuda, dt):
    """Inside torch.autocast at the canonical latent, s = 3: at most 2 (1 + 2|s|) times the single-style 16-bit loop's
    error against float64 on the same inputs (the larger of the target's and the base's).
    Measured on an MI355X: fp16 1.81e-4 against 6.87e-5 / 7.52e-5 (target / base); bf16 1.28e-3 against 6.25e-4 /
    6.03e-4."""
    from ldm_amd.engine import UNetEngine
    s = 3.0
    z, tgt, base = inputs(2, 16, 64, 401)
    eng = UNetEngine(ctx["ldm"].unet)
    with torch.autocast("cuda", dtype=dt):
        assert eng.step_dtype() == (1 if dt == torch.float16 else 2)
        x, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, z, tgt, base=base, scale=s)
        xt, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, z, tgt)
        xb, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, z, base)
    want, _, _ = GR.sample(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), tgt, base, s)
    wt, _, _ = GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), tgt)
    wb, _, _ = GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), base)
    e, e_t, e_b = rel_err(npy(x), want), rel_err(npy(xt), wt), rel_err(npy(xb), wb)
    print(f"{dt}: guided s=3 {e:.3e}; single style: target {e_t:.3e}, base {e_b:.3e}")
    assert e <= 2.0 * (1.0 + 2.0 * s) * max(e_t, e_b)


# ---- 5. determinism, capture, split ----------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
def test_run_twice_and_capture(ctx, cuda, solver, eta):
    from ldm_amd.engine import GraphedDDIM
    B = 4
    z, tgt, base = inputs(B, 16, 64, 501)
    eng = engine(ctx, "default")
    s_a, s_b = torch.tensor([3.0, 0.5, -1.25, 2.0]), 1.75
    a = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=s_a)
    a2 = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=s_a)
    for u, v in zip(a, a2):
        assert torch.equal(u, v)
    b = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=s_b)
    # a captured loop equals the eager call; after rewriting the static scale buffer it equals a fresh eager call
    times = ctx["times"]
    fd = ctx["ldm"].noise_scheduler
    tt = torch.from_numpy(times)
    coef = (fd.multistep_coefs(tt) if solver != "ddim" else fd.reverse_coefs(tt)).to(cuda)
    t_table = tt[:-1].view(STEPS, 1).expand(STEPS, B).contiguous().to(cuda)
    with torch.no_grad():
        gd = GraphedDDIM(eng, z.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, logs=True,
                         solver="msolver" if solver != "ddim" else "ddim",
                         base=(base[0].to(cuda), base[1].to(cuda), None, None), guidance_scale=s_a)
        r = gd.replay().clone()
        torch.cuda.synchronize()
        assert torch.equal(r, a[0]) and torch.equal(gd.x0_logs, a[1]) and torch.equal(gd.eps_logs, a[2])
        gd.set_guidance_scale(s_b)
        r = gd.replay().clone()
        torch.cuda.synchronize()
        assert torch.equal(r, b[0]) and torch.equal(gd.x0_logs, b[1]) and torch.equal(gd.eps_logs, b[2])


@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
def test_split_two_equals_split_one_bitwise(ctx, cuda, solver, eta):
    """Sub-batch chains at B = 4: the log strides and the base / scale slices, bitwise.

    The plain loop does not have this property at the canonical latent (printed below: B = 8 in one chain against two
    chains of 4 differs at 1.8e-7, because the K/V projection of CA1 gets another kernel kind at the smaller batch,
    which UNetEngine.ddim_loop documents as "the same up to fp32 summation order").  The guided loop's chains run the
    whole batch's plans instead (UNetEngine._guided_weights), so each sample's arithmetic is the one split = 1 gives
    it; a captured split loop replays the same values."""
    from ldm_amd.engine import GraphedDDIM
    B = 4
    z, tgt, base = inputs(B, 16, 64, 501)
    eng = engine(ctx, "default")
    s_a = torch.tensor([3.0, 0.5, -1.25, 2.0])
    a = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=s_a)
    # (printed beside it: the plain loop at the same internal batches, B = 8 in one chain against two chains of 4)
    two = lambda t: torch.cat([t, t])      # noqa: E731
    p1 = run(ctx, cuda, eng, solver, eta, two(z), (two(tgt[0]), two(tgt[1])))
    p2 = run(ctx, cuda, eng, solver, eta, two(z), (two(tgt[0]), two(tgt[1])), split=2)
    print(f"plain loop B 8, split 2 against 1: x {rel_err(npy(p2[0]), npy(p1[0])):.2e}, bitwise {torch.equal(p1[0], p2[0])}")
    c = run(ctx, cuda, eng, solver, eta, z, tgt, base=base, scale=s_a, split=2)
    for name, u, v in zip(("x", "x0 logs", "eps logs"), a, c):
        print(f"split 2 against 1, {name}: {rel_err(npy(v), npy(u)):.2e}")
    for name, u, v in zip(("x", "x0 logs", "eps logs"), a, c):
        assert rel_err(npy(v), npy(u)) <= FOLD_TOL, name
    for name, u, v in zip(("x", "x0 logs", "eps logs"), a, c):
        assert torch.equal(u, v), name
    tt = torch.from_numpy(ctx["times"])
    fd = ctx["ldm"].noise_scheduler
    coef = (fd.multistep_coefs(tt) if solver != "ddim" else fd.reverse_coefs(tt)).to(cuda)
    t_table = tt[:-1].view(STEPS, 1).expand(STEPS, B).contiguous().to(cuda)
    with torch.no_grad():
        gd = GraphedDDIM(eng, z.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, logs=True, split=2,
                         solver="msolver" if solver != "ddim" else "ddim",
                         base=(base[0].to(cuda), base[1].to(cuda), None, None), guidance_scale=s_a)
        r = gd.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(r, a[0]) and torch.equal(gd.x0_logs, a[1]) and torch.equal(gd.eps_logs, a[2])


# ---- 6. a mix as the target, the tiled single style as the base ------------------------------------------------------
def test_mix_target_with_a_tiled_base(ctx, cuda):
    import stylemix_ref as MR
    ldm, M = ctx["ldm"], ctx["M"]
    B, H, W, s = 2, 16, 16, 2.0
    g = torch.Generator().manual_seed(601)
    z = torch.randn(B, 32, H, W, generator=g)
    specs = torch.rand(B, 2, 1, 128, 128, generator=g).to(cuda)
    base_spec = torch.rand(B, 1, 128, 128, generator=g).to(cuda)
    with torch.no_grad():
        emb = ldm.encode_styles(specs, [0.25, 0.75])
        bemb = M.LDM.tile_embedding(ldm.style_encoder(base_spec), 2)
        assert emb["refs"] == 2 and tuple(bemb["s5"].shape) == tuple(emb["s5"].shape) and bemb["key_bias5"] is None
        x, logs = ldm.style_conditioned_sample(z.to(cuda), emb, steps=STEPS, t_start=99, guidance_scale=s,
                                               base_embedding=bemb)
        xt, _ = ldm.style_conditioned_sample(z.to(cuda), emb, steps=STEPS, t_start=99)
        xb, _ = ldm.style_conditioned_sample(z.to(cuda), bemb, steps=STEPS, t_start=99)
    torch.cuda.synchronize()
    L2, L1 = (H // 4) * (W // 4), (H // 8) * (W // 8)
    tgt = (emb["s5"].cpu(), emb["s6"].cpu(), MR.key_weights([0.25, 0.75], B, 2, L2), MR.key_weights([0.25, 0.75], B, 2, L1))
    base = (bemb["s5"].cpu(), bemb["s6"].cpu(), MR.key_weights([0.5, 0.5], B, 2, L2), MR.key_weights([0.5, 0.5], B, 2, L1))
    want, x0s, _ = GR.sample(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), tgt, base, s)
    wt, _, _ = GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), tgt)
    wb, _, _ = GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(z), base)
    e, e_t, e_b = rel_err(npy(x), want), rel_err(npy(xt), wt), rel_err(npy(xb), wb)
    bar = bars(s, e_t, e_b)
    print(f"mix R 2 (0.25, 0.75) against the tiled base, s {s}: {e:.2e}; plain e_t {e_t:.2e} e_b {e_b:.2e}; bar {bar:.2e}")
    assert e <= bar and rel_err(npy(logs["pred_x0"][-1]), x0s[-1]) <= bar
    with pytest.raises(ValueError, match="key counts"):
        ldm.style_conditioned_sample(z.to(cuda), emb, steps=STEPS, t_start=99, guidance_scale=s,
                                     base_embedding=ldm.style_encoder(base_spec))


# ---- 7. the stand-alone kernel and the per-layer fallback ------------------------------------------------------------
def test_guide_eps_kernel(cuda):
    from ldm_amd import ops
    g = torch.Generator().manual_seed(701)
    e_t, e_b = torch.randn(3, 5, 7, 9, generator=g), torch.randn(3, 5, 7, 9, generator=g)
    s = torch.tensor([3.7, -1.25, 0.0])
    got = ops.guide_eps(e_t.to(cuda), e_b.to(cuda), s.to(cuda))
    torch.cuda.synchronize()
    want = GR.guide(npy(e_t), npy(e_b), s.double().numpy())
    e = rel_err(npy(got), want)
    print(f"ldm_guide_eps: {e:.2e}")
    assert e <= 1e-6
    # the definition's op sequence in fp32, one rounding each
    assert torch.equal(got.cpu(), e_b + s.view(3, 1, 1, 1) * (e_t - e_b))
    assert torch.equal(ops.guide_eps(e_t.to(cuda), e_t.to(cuda), s.to(cuda)).cpu(), e_t)      # d = 0 exactly
    with pytest.raises(ValueError):
        ops.guide_eps(e_t.to(cuda), e_b.to(cuda), s[:2].to(cuda))


@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
def test_per_layer_fallback(ctx, cuda, solver, eta):
    """A latent width the engine does not take: two per-layer UNet calls, ldm_guide_eps, then the update kernel."""
    M = ctx["M"]
    assert not M.UNetEngine.supports(4)
    torch.manual_seed(2)
    ldm4 = M.LDM(4, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm4.state_dict().items()}
    z, tgt, base = inputs(2, 16, 16, 702, C=4)
    sv = np.array([3.0, 0.5])
    emb = lambda m: {"s5": m[0].to(cuda), "s6": m[1].to(cuda)}      # noqa: E731
    with torch.no_grad():
        x, logs = ldm4.style_conditioned_sample(z.to(cuda), emb(tgt), steps=STEPS, t_start=99, solver=solver, eta=eta,
                                                guidance_scale=torch.from_numpy(sv), base_embedding=emb(base))
        xt, _ = ldm4.style_conditioned_sample(z.to(cuda), emb(tgt), steps=STEPS, t_start=99, solver=solver, eta=eta)
        xb, _ = ldm4.style_conditioned_sample(z.to(cuda), emb(base), steps=STEPS, t_start=99, solver=solver, eta=eta)
    torch.cuda.synchronize()
    want, x0s, _ = GR.sample(sd64, ctx["ab"], ctx["times"], npy(z), tgt, base, sv, solver, eta)
    wt, _, _ = GR.sample_plain(sd64, ctx["ab"], ctx["times"], npy(z), tgt, solver, eta)
    wb, _, _ = GR.sample_plain(sd64, ctx["ab"], ctx["times"], npy(z), base, solver, eta)
    e, e_t, e_b = rel_err(npy(x), want), rel_err(npy(xt), wt), rel_err(npy(xb), wb)
    bar = bars(sv, e_t, e_b)
    print(f"per-layer fallback {solver} eta {eta}: {e:.2e}; plain e_t {e_t:.2e} e_b {e_b:.2e}; bar {bar:.2e}")
    assert e <= bar and rel_err(npy(logs["pred_x0"][1]), x0s[1]) <= bar


# ---- 8. the public methods -------------------------------------------------------------------------------------------
def test_content_style_transfer_and_transfer_recording(ctx, cuda):
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    from models.transfer import transfer_recording
    ldm = ctx["ldm"]
    content = torch.from_numpy(AR.test_signal(900 * 512)).float().to(cuda)      # 901 frames: two windows of 512 / 64
    style = torch.from_numpy(AR.test_signal(520 * 512, variant=1)).float().to(cuda)
    other = torch.from_numpy(AR.test_signal(520 * 512, variant=2)).float().to(cuda)
    kw = dict(frames=512, overlap=64, n_iter=2, nnls_iters=2, seed=4, num_timesteps=STEPS, solver="dpmpp2m")
    x, ref = LF.mel_windows(A.melspectrogram(content), 512, 64)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 512, 0)
    xo, _ = LF.mel_windows(A.melspectrogram(other), 512, 0)
    assert x.shape[0] == 2
    st2 = xs[:1].expand(2, -1, -1, -1).contiguous()
    noise = torch.randn((2, 32, 16, 64), generator=torch.Generator().manual_seed(4)).to(cuda)
    ckw = dict(t_start=99, steps=STEPS, solver="dpmpp2m", noise=noise)
    with torch.no_grad():
        plain, _ = ldm.content_style_transfer(x, st2, **ckw)
        g_default, _ = ldm.content_style_transfer(x, st2, guidance_scale=2.0, **ckw)
        g_content, _ = ldm.content_style_transfer(x, st2, guidance_scale=2.0, base_style=x, **ckw)
        g_other, _ = ldm.content_style_transfer(x, st2, guidance_scale=2.0, base_style=xo[:1].expand(2, -1, -1, -1), **ckw)
        same, _ = ldm.content_style_transfer(x, st2, guidance_scale=1.0, base_style=None, **ckw)
    assert torch.equal(g_default, g_content)                  # base None at a scale other than 1: the content itself
    assert torch.equal(same, plain)                            # scale 1, no base: the unguided path
    assert not torch.equal(g_default, plain) and not torch.equal(g_other, g_default)
    assert bool(torch.isfinite(g_default).all()) and bool(torch.isfinite(g_other).all())
    # the whole recording
    res = transfer_recording(ldm, content, style, guidance_scale=2.0, **kw)
    res_c = transfer_recording(ldm, content, style, guidance_scale=2.0, base_style="content", **kw)
    assert res.N == 2 and torch.equal(res.windows_out, g_content) and torch.equal(res_c.windows_out, g_content)
    mel = LF.stitch_windows(g_content, ref, 64, 901)
    assert torch.equal(res.mel_power, mel)
    assert torch.equal(res.audio, A.mel_to_audio(mel, seed=4, length=900 * 512, n_iter=2, nnls_iters=2))
    assert torch.equal(res_c.audio, res.audio)
    res_o = transfer_recording(ldm, content, style, guidance_scale=2.0, base_style=other, **kw)
    assert torch.equal(res_o.windows_out, g_other)
    res0 = transfer_recording(ldm, content, style, **kw)       # without the new arguments: the unguided method
    assert torch.equal(res0.windows_out, plain)
    with pytest.raises(ValueError, match="solver"):
        transfer_recording(ldm, content, style, guidance_scale=2.0, **dict(kw, solver=None))
    with pytest.raises(ValueError, match="finite"):
        transfer_recording(ldm, content, style, guidance_scale=float("nan"), **kw)


# ---- 9. errors of the C entry points ---------------------------------------------------------------------------------
def test_c_abi_errors(ctx, cuda):
    import ctypes
    from ldm_amd import _lib as L
    from ldm_amd import ops
    eng = engine(ctx, "default")
    B, H, W = 2, 8, 16
    z, tgt, base = inputs(B, H, W, 901)
    shape = eng.shape(B, 32, H, W)
    w = eng.weights(eng.shape(2 * B, 32, H, W))
    ws = eng.workspace(shape, cuda, STEPS, guided=True)
    assert ws.numel() > eng.workspace(shape, cuda, STEPS).numel()

    def size(wts, **fields):
        return int(L.load().ldm_sample_workspace_floats(ctypes.byref(shape), ctypes.byref(wts), ctypes.byref(L.SampleArgs(**fields))))

    assert size(w, nsteps=-1, s5_base=1, s6_base=1, guide_scale=1) < 0
    x = z.to(cuda).clone()
    d = [t.to(cuda) for t in (*tgt, *base)]
    tt = torch.from_numpy(ctx["times"])
    fd = ctx["ldm"].noise_scheduler
    t_table = tt[:-1].view(STEPS, 1).expand(STEPS, B).contiguous().to(cuda)
    scale = torch.ones(B, device=cuda)
    x0l = torch.empty((STEPS,) + tuple(z.shape), device=cuda)

    def call(solver, s5b, s6b, sc, coef, wsp=None, wts=w):
        a = L.SampleArgs(solver=L.SOLVER[solver], nsteps=STEPS, eta=0.0, x=x.data_ptr(), s5=d[0].data_ptr(),
                         s6=d[1].data_ptr(), s5_base=s5b, s6_base=s6b, guide_scale=sc, t_table=t_table.data_ptr(),
                         coef_table=coef.data_ptr(), x0_logs=x0l.data_ptr(), workspace=wsp or ws.data_ptr(),
                         stream=ops.stream_handle())
        L.call("ldm_sample", ctypes.byref(shape), ctypes.byref(wts), ctypes.byref(a))

    c4, c8 = fd.reverse_coefs(tt).to(cuda), fd.multistep_coefs(tt).to(cuda)
    for name, coef in (("ddim", c4), ("msolver", c8)):
        with pytest.raises(L.LDMError, match="base"):
            call(name, None, d[3].data_ptr(), scale.data_ptr(), coef)
        with pytest.raises(L.LDMError, match="base"):
            call(name, d[2].data_ptr(), None, scale.data_ptr(), coef)
        with pytest.raises(L.LDMError, match="scale"):
            call(name, d[2].data_ptr(), d[3].data_ptr(), None, coef)
    with pytest.raises(L.LDMError):
        L.call("ldm_guide_eps", x.data_ptr(), x.data_ptr(), None, 16, B, x.data_ptr(), ops.stream_handle())
    # a workspace sized for the unguided loop, as an allocation of its own (the entry asks the runtime for the
    # extent of the allocation that holds the pointer; torch's caching allocator would hand out part of a larger one)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], ctypes.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [ctypes.c_void_p], ctypes.c_int
    w1 = eng.weights(shape)
    n_small = size(w1, nsteps=STEPS)
    assert 0 < n_small < ws.numel()
    short = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(short), n_small * 4) == 0
    try:
        for name, coef in (("ddim", c4), ("msolver", c8)):
            with pytest.raises(L.LDMError, match="workspace"):
                call(name, d[2].data_ptr(), d[3].data_ptr(), scale.data_ptr(), coef, short.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipFree(short) == 0
    # the plain loop (no base, no keep) is held to its size too: one float short is an error, not an overrun
    assert hip.hipMalloc(ctypes.byref(short), (n_small - 1) * 4) == 0
    try:
        with pytest.raises(L.LDMError, match="workspace"):
            call("ddim", None, None, None, c4, short.value, w1)
    finally:
        torch.cuda.synchronize()
        assert hip.hipFree(short) == 0
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), z)          # nothing ran
    # the good calls still work afterwards: the plain one on a workspace of its size, then the guided one
    call("ddim", None, None, None, c4, eng.workspace(shape, cuda, STEPS).data_ptr(), w1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x.cpu(), z)
    x.copy_(z.to(cuda))
    call("ddim", d[2].data_ptr(), d[3].data_ptr(), scale.data_ptr(), c4)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x.cpu(), z)
