"""GPU: joint sampling of overlapping windows (the seam fuse before step 0 and after every step's update) from the
stand-alone kernel up to transfer_recording, against the float64 yardstick tests/seam_ref.py and the oracle's UNet.

Bars.  The fuse alone is held bitwise to the definition's fp32 operation sequence in torch; B = 1 with a seam is held
bitwise to the plain loop; after a joint loop both sides of every seam are bitwise equal.  Against float64 a joint
loop may cost at most twice the error of the corresponding loop without the seam on the same inputs, measured in the
same test (the two loops' trajectories differ), and never more than 1e-4, the loops' existing bar (the keep's rule,
tests/test_gpu_regional.py, whose loop list, inputs and helpers are used here)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR               # noqa: E402
import guidance_ref as GR            # noqa: E402
import regional_ref as RR            # noqa: E402
import seam_ref as SM                # noqa: E402
import solver_ref as SR              # noqa: E402
import test_gpu_regional as TR       # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN_TOL = TR.PLAIN_TOL
SOLVERS, SOLVER_IDS = TR.SOLVERS, TR.SOLVER_IDS
STEPS = 4
LOOPS, LOOP_IDS = TR.LOOPS, TR.LOOP_IDS
npy, engine, inputs, coef_tables, errs3 = TR.npy, TR.engine, TR.inputs, TR.coef_tables, TR.errs3
assert TR.STEPS == STEPS


def seam_of(W):
    """The seam width the loop tests use at a latent width: 8 columns at the canonical 64, 3 (odd, under W / 2) at 16."""
    return 8 if W == 64 else 3


@pytest.fixture(scope="module")
def ctx(cuda):
    """The model (never modified), its float64 state dict and schedule."""
    import models.model as M
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm.state_dict().items()}
    return dict(M=M, ldm=ldm, sd64=sd64, ab=SR.alpha_bar(ldm.num_timesteps), times=SR.sample_times(99, STEPS), cache={})


def run(ctx, cuda, eng, solver, eta, x_in, tgt, ov=0, keep=None, base=None, scale=1.0, split=1):
    """One loop on the engine with seam_cols = ov.  keep = (z0, n0, w) or None.  Returns (x, x0_logs, eps_logs)."""
    B = x_in.shape[0]
    tt, fd, coef, t_table = coef_tables(ctx, cuda, solver, B)
    x = x_in.to(cuda).clone()
    x0l = torch.full((STEPS,) + tuple(x_in.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    kw = dict(split=split)
    if ov:
        kw.update(seam_cols=ov)
    if base is not None:
        kw.update(base=(base[0].to(cuda), base[1].to(cuda), None, None), guidance_scale=scale)
    if keep is not None:
        kw.update(keep=dict(z0=keep[0].to(cuda), n0=keep[1].to(cuda), w=keep[2].to(cuda), coefs=fd.keep_coefs(tt, True)))
    with torch.no_grad():
        if solver == "ddim":
            eng.ddim_loop(x, tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, x0l, epl, **kw)
        else:
            eng.msolver_loop(x, tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, x0l, epl, **kw)
    torch.cuda.synchronize()
    return x, x0l, epl


def fuse_fp32(x, ov):
    """The definition's fp32 operation sequence in torch (CPU), one rounding per operation."""
    x = x.clone()
    B, _, _, W = x.shape
    w = (torch.arange(ov, dtype=torch.float32) + 1.0) / torch.tensor(float(ov + 1), dtype=torch.float32)
    for b in range(B - 1):
        a, q = x[b, :, :, W - ov:].clone(), x[b + 1, :, :, :ov].clone()
        d = q - a
        p = w * d
        m = a + p
        x[b, :, :, W - ov:] = m
        x[b + 1, :, :, :ov] = m
    return x


# ---- 1. the stand-alone kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ov", [((3, 32, 8, 16), 1), ((3, 32, 8, 16), 3), ((3, 32, 8, 16), 8), ((2, 32, 16, 64), 8)],
                         ids=["3x8x16-ov1", "3x8x16-ov3", "3x8x16-ov8", "2x16x64-ov8"])
def test_seam_fuse_kernel_bitwise(cuda, shape, ov):
    """ov = 8 = W / 2 on the 8 x 16 latent: the middle window's two seams abut."""
    from ldm_amd import ops
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1000 + ov + shape[3]))
    got = ops.seam_fuse_(x.to(cuda).clone(), ov).cpu()
    torch.cuda.synchronize()
    want = fuse_fp32(x, ov)
    assert torch.equal(got, want)
    B, W = shape[0], shape[3]
    for b in range(B - 1):
        assert torch.equal(got[b, :, :, W - ov:], got[b + 1, :, :, :ov])
    assert not torch.equal(got, x)
    e = rel_err(npy(got), SM.fuse(npy(x), ov))
    print(f"ldm_seam_fuse {shape} ov {ov}: {e:.2e}")
    assert e <= 1e-6
    one = x[:1].to(cuda).clone()
    assert torch.equal(ops.seam_fuse_(one, ov).cpu(), x[:1])                 # B = 1 leaves x bitwise
    for bad in (0, W // 2 + 1):
        with pytest.raises(ValueError):
            ops.seam_fuse_(x.to(cuda), bad)


# ---- 2. B = 1 with a seam is the plain loop --------------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_one_window_with_a_seam_is_the_plain_loop_bitwise(ctx, cuda, kind, B, H, W, solver, eta):
    eng = engine(ctx, kind)
    x, _, _, tgt, _ = inputs(ctx, 1, H, W, 1100 + H + W)
    p = run(ctx, cuda, eng, solver, eta, x, tgt)
    j = run(ctx, cuda, eng, solver, eta, x, tgt, ov=seam_of(W))
    for name, u, v in zip(("x", "x0 logs", "eps logs"), p, j):
        assert torch.equal(u, v), name


# ---- 3. agreement across every seam ----------------------------------------------------------------------------------
def raw_sample(eng, cuda, x, tgt, t_table, coef, nsteps, seam_cols, x0l):
    """ldm_sample through the C ABI with the given nsteps / seam_cols on the engine's weights and workspace."""
    from ldm_amd import _lib as L
    from ldm_amd import ops
    B, C, H, W = x.shape
    shape = eng.shape(B, C, H, W)
    w = eng.weights(shape)
    ws = eng.workspace(shape, cuda, STEPS)
    a = L.SampleArgs(solver=L.SOLVER["ddim"], nsteps=nsteps, eta=0.0, seam_cols=seam_cols, x=x.data_ptr(),
                     s5=tgt[0].data_ptr(), s6=tgt[1].data_ptr(), t_table=t_table.data_ptr(), coef_table=coef.data_ptr(),
                     x0_logs=x0l.data_ptr(), workspace=ws.data_ptr(), stream=ops.stream_handle())
    L.call("ldm_sample", ctypes.byref(shape), ctypes.byref(w), ctypes.byref(a))


@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
@pytest.mark.parametrize("B,H,W,ov", [(3, 8, 16, 3), (2, 16, 64, 8)], ids=["3x8x16-ov3", "2x16x64-ov8"])
def test_seams_agree_bitwise_and_feed_back(ctx, cuda, B, H, W, ov, solver, eta):
    eng = engine(ctx, "default")
    x, _, _, tgt, _ = inputs(ctx, B, H, W, 1200 + H + W)
    p = run(ctx, cuda, eng, solver, eta, x, tgt)
    j = run(ctx, cuda, eng, solver, eta, x, tgt, ov=ov)
    for b in range(B - 1):
        assert torch.equal(j[0][b, :, :, W - ov:], j[0][b + 1, :, :, :ov]), f"seam {b}"
        assert not torch.equal(p[0][b, :, :, W - ov:], p[0][b + 1, :, :, :ov])       # (the plain loop's do not)
    # the fuse fed back into the trajectory: columns outside every seam moved too, in every row
    assert ov < W - ov
    for b in range(B):
        assert not torch.equal(j[0][b, :, :, ov:W - ov], p[0][b, :, :, ov:W - ov]), f"row {b}"
    # the logs are each window's own prediction: they do not agree across the seam
    assert not torch.equal(j[1][-1][0, :, :, W - ov:], j[1][-1][1, :, :, :ov])
    assert bool(torch.isfinite(j[0]).all()) and bool(torch.isfinite(j[1]).all()) and bool(torch.isfinite(j[2]).all())
    if solver == "ddim":      # nsteps = 0 returns at once: the state is not fused either
        tt, fd, coef, t_table = coef_tables(ctx, cuda, "ddim", B)
        xs = x.to(cuda).clone()
        x0l = torch.empty((STEPS,) + tuple(x.shape), device=cuda)
        raw_sample(eng, cuda, xs, [t.to(cuda) for t in tgt], t_table, coef, 0, ov, x0l)
        torch.cuda.synchronize()
        assert torch.equal(xs.cpu(), x)


# ---- 4. against float64 ----------------------------------------------------------------------------------------------
def plain_result(ctx, cuda, kind, B, H, W, solver, eta):
    """The plain loop's errors against float64 (final x, x0 logs, eps logs) on the inputs of test 4, computed once per
    configuration, shared, never modified."""
    key = (kind, B, H, W, solver, eta)
    if key not in ctx["cache"]:
        x, _, _, tgt, _ = inputs(ctx, B, H, W, 1300 + H + W)
        got = run(ctx, cuda, engine(ctx, kind), solver, eta, x, tgt)
        ctx["cache"][key] = errs3(got, GR.sample_plain(ctx["sd64"], ctx["ab"], ctx["times"], npy(x), tgt, solver, eta))
    return ctx["cache"][key]


@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,B,H,W", LOOPS, ids=LOOP_IDS)
def test_joint_loop_against_float64(ctx, cuda, kind, B, H, W, solver, eta):
    """x and both logs, each held to min(2 e_plain, 1e-4) of the same quantity.  Measured values: DESIGN.md 7i."""
    e_plain = plain_result(ctx, cuda, kind, B, H, W, solver, eta)
    x, _, _, tgt, _ = inputs(ctx, B, H, W, 1300 + H + W)
    ov = seam_of(W)
    got = run(ctx, cuda, engine(ctx, kind), solver, eta, x, tgt, ov=ov)
    e = errs3(got, SM.sample(ctx["sd64"], ctx["ab"], ctx["times"], npy(x), tgt, ov, solver, eta))
    print(f"{kind} B{B} {H}x{W} ov {ov} {solver} eta {eta}: joint x {e[0]:.2e} x0 {e[1]:.2e} eps {e[2]:.2e}; plain x "
          f"{e_plain[0]:.2e} x0 {e_plain[1]:.2e} eps {e_plain[2]:.2e}")
    for q in range(3):
        assert e[q] <= min(2.0 * e_plain[q], PLAIN_TOL), ("x", "x0 logs", "eps logs")[q]


# ---- 5. composed with the guidance and the keep ----------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", SOLVERS, ids=SOLVER_IDS)
@pytest.mark.parametrize("kind,H,W", [("default", 8, 16), ("folded-general", 16, 16), ("unfolded", 16, 16)],
                         ids=["step-3x8x16", "folded-general-3x16x16", "unfolded-3x16x16"])
def test_guided_keep_seam_against_float64(ctx, cuda, kind, H, W, solver, eta):
    """Guidance at scale 3 + a mixed keep mask + the seam at B = 3; the bar is the guided keep loop's own error
    without the seam on the same inputs.  The engine's doubled state is [targets 0..2 | bases 0..2]: row 2 of the target
    half and row 0 of the base half are neighbours in memory but not windows of one canvas.  A fuse across them would
    move the target half's last window and the base half's first away from the yardstick (which fuses B rows, once,
    and evaluates both styles on that one state), so the float64 comparison below is also the check that they were not
    fused."""
    B, ov = 3, 3
    x, z0, n0, tgt, base = inputs(ctx, B, H, W, 1400 + H + W)
    w = TR.mask(B, H, W)
    eng = engine(ctx, kind)
    args = (ctx["sd64"], ctx["ab"], ctx["times"], npy(x))
    e_g = errs3(run(ctx, cuda, eng, solver, eta, x, tgt, keep=(z0, n0, w), base=base, scale=3.0),
                RR.sample(*args, tgt, npy(z0), npy(n0), npy(w), solver, eta, base=base, s=3.0))
    got = run(ctx, cuda, eng, solver, eta, x, tgt, ov=ov, keep=(z0, n0, w), base=base, scale=3.0)
    e = errs3(got, SM.sample(*args, tgt, ov, solver, eta, keep=(npy(z0), npy(n0), npy(w)), base=base, s=3.0))
    print(f"{kind} B{B} {H}x{W} ov {ov} {solver} eta {eta} guided + keep: joint x {e[0]:.2e} x0 {e[1]:.2e} eps {e[2]:.2e}; "
          f"without the seam x {e_g[0]:.2e} x0 {e_g[1]:.2e} eps {e_g[2]:.2e}")
    for b in range(B - 1):
        assert torch.equal(got[0][b, :, :, W - ov:], got[0][b + 1, :, :, :ov]), f"seam {b}"
    for q in range(3):
        assert e[q] <= min(2.0 * e_g[q], PLAIN_TOL), ("x", "x0 logs", "eps logs")[q]


# ---- 6. 16-bit operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16_bit_operands(ctx, cuda, dt):
    """Inside torch.autocast at the canonical latent: at most twice the plain 16-bit loop's error against float64 on
    the same inputs (the fuse is fp32 on the fp32 state and adds no 16-bit rounding)."""
    from ldm_amd.engine import UNetEngine
    x, _, _, tgt, _ = inputs(ctx, 2, 16, 64, 1501)
    eng = UNetEngine(ctx["ldm"].unet)
    with torch.autocast("cuda", dtype=dt):
        assert eng.step_dtype() == (1 if dt == torch.float16 else 2)
        xj, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, x, tgt, ov=8)
        xp, _, _ = run(ctx, cuda, eng, "dpmpp2m", 0.0, x, tgt)
    args = (ctx["sd64"], ctx["ab"], ctx["times"], npy(x))
    wj, _, _ = SM.sample(*args, tgt, 8)
    wp, _, _ = GR.sample_plain(*args, tgt)
    e, e_p = rel_err(npy(xj), wj), rel_err(npy(xp), wp)
    print(f"{dt}: joint {e:.3e}; plain {e_p:.3e}")
    assert torch.equal(xj[0, :, :, 56:], xj[1, :, :, :8])
    assert e <= 2.0 * e_p


# ---- 7. capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,eta", [("ddim", 1.0), ("dpmpp2m", 0.0)], ids=["ddim-eta1", "dpmpp2m"])
def test_capture(ctx, cuda, solver, eta):
    from ldm_amd.engine import GraphedDDIM
    B, ov = 4, 8
    x, _, _, tgt, _ = inputs(ctx, B, 16, 64, 1601)
    eng = engine(ctx, "default")
    j = run(ctx, cuda, eng, solver, eta, x, tgt, ov=ov)
    p = run(ctx, cuda, eng, solver, eta, x, tgt)
    assert not torch.equal(j[0], p[0])
    tt, fd, coef, t_table = coef_tables(ctx, cuda, solver, B)
    kind = "msolver" if solver != "ddim" else "ddim"
    with torch.no_grad():
        gd = GraphedDDIM(eng, x.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, logs=True, solver=kind,
                         seam_cols=ov)
        for _ in range(2):
            r = gd.replay().clone()
            torch.cuda.synchronize()
            assert torch.equal(r, j[0]) and torch.equal(gd.x0_logs, j[1]) and torch.equal(gd.eps_logs, j[2])
        g0 = GraphedDDIM(eng, x.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, logs=True, solver=kind)
        r = g0.replay().clone()
        torch.cuda.synchronize()
        assert torch.equal(r, p[0]) and torch.equal(g0.x0_logs, p[1]) and torch.equal(g0.eps_logs, p[2])
        with pytest.raises(ValueError, match="split"):
            GraphedDDIM(eng, x.to(cuda), tgt[0].to(cuda), tgt[1].to(cuda), t_table, coef, eta, solver=kind, split=2,
                        seam_cols=ov)


# ---- 8. errors -------------------------------------------------------------------------------------------------------
def test_split_and_c_abi_errors(ctx, cuda):
    from ldm_amd import _lib as L
    eng = engine(ctx, "default")
    B, H, W = 2, 8, 16
    xin, _, _, tgt, _ = inputs(ctx, B, H, W, 1701)
    with pytest.raises(ValueError, match="split"):
        run(ctx, cuda, eng, "ddim", 0.0, xin, tgt, ov=3, split=2)
    for bad in (-1, W // 2 + 1):
        with pytest.raises(ValueError, match="seam_cols"):
            run(ctx, cuda, eng, "ddim", 0.0, xin, tgt, ov=bad)
    shape = eng.shape(B, 32, H, W)
    w = eng.weights(shape)

    def size(**fields):
        return int(L.load().ldm_sample_workspace_floats(ctypes.byref(shape), ctypes.byref(w), ctypes.byref(L.SampleArgs(**fields))))

    assert size(nsteps=STEPS, seam_cols=3) == size(nsteps=STEPS) > 0
    assert size(nsteps=STEPS, seam_cols=3, z0=1, n0=1, keep=1, keep_coef=1) == size(nsteps=STEPS, z0=1, n0=1, keep=1, keep_coef=1)
    tt, fd, coef, t_table = coef_tables(ctx, cuda, "ddim", B)
    x = xin.to(cuda).clone()
    d = [t.to(cuda) for t in tgt]
    x0l = torch.empty((STEPS,) + tuple(xin.shape), device=cuda)
    for bad in (-1, W // 2 + 1):
        with pytest.raises(L.LDMError, match="seam_cols"):
            raw_sample(eng, cuda, x, d, t_table, coef, STEPS, bad, x0l)
    with pytest.raises(L.LDMError, match="seam_cols"):
        L.call("ldm_seam_fuse", x.data_ptr(), B, 32, H, W, W // 2 + 1, None)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), xin)          # nothing ran
    raw_sample(eng, cuda, x, d, t_table, coef, STEPS, W // 2, x0l)           # the widest legal seam works afterwards
    torch.cuda.synchronize()
    j, _, _ = run(ctx, cuda, eng, "ddim", 0.0, xin, tgt, ov=W // 2)
    assert torch.equal(x, j) and torch.equal(x[0, :, :, W // 2:], x[1, :, :, :W // 2])


# ---- 9. end to end ---------------------------------------------------------------------------------------------------
def seam_db_gap(windows, ref_db, overlap, max_db=80.0):
    """Mean |dB difference| of the two decoded windows over each overlap (what the crossfade has to reconcile)."""
    y = windows[:, 0].clamp(0, 1) * max_db - max_db + ref_db.view(-1, 1, 1)
    return [float((y[n, :, -overlap:] - y[n + 1, :, :overlap]).abs().mean()) for n in range(y.shape[0] - 1)]


def test_transfer_recording_joint(ctx, cuda):
    """Three windows of 128 frames sharing 32 (W = 16, ov = 4).  With batch_size = 2 the groups are windows [0, 1]
    (a joint pair) and [2] (alone: the plain loop on the canvas noise); the seam between windows 1 and 2 is not fused,
    so both windows touching it differ from the one-canvas result.  Window 0 is coupled to window 1 through their fused
    seam after every step, so it follows window 1's change: it is held to the direct joint call on the pair."""
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    from models.transfer import HOP, transfer_recording
    ldm = ctx["ldm"]
    content = torch.from_numpy(AR.test_signal(300 * 512)).float().to(cuda)      # 301 frames: three windows of 128 / 32
    style = torch.from_numpy(AR.test_signal(140 * 512, variant=1)).float().to(cuda)
    kw = dict(frames=128, overlap=32, n_iter=2, nnls_iters=2, seed=4, num_timesteps=STEPS, solver="dpmpp2m")
    x, ref = LF.mel_windows(A.melspectrogram(content), 128, 32)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 128, 0)
    assert x.shape[0] == 3 and HOP == 512
    st3 = xs[:1].expand(3, -1, -1, -1).contiguous()
    noise = LF.noise_windows(3, 32, 16, 16, 4, 4).to(cuda)
    ckw = dict(t_start=99, steps=STEPS, solver="dpmpp2m")
    with torch.no_grad():
        direct, _ = ldm.content_style_transfer(x, st3, noise=noise, seam_overlap=32, **ckw)
        pair, _ = ldm.content_style_transfer(x[:2], st3[:2], noise=noise[:2], seam_overlap=32, **ckw)
        last, _ = ldm.content_style_transfer(x[2:], st3[2:], noise=noise[2:], **ckw)
        res3 = transfer_recording(ldm, content, style, joint=True, batch_size=3, **kw)
        res2 = transfer_recording(ldm, content, style, joint=True, batch_size=2, **kw)
        res_off = transfer_recording(ldm, content, style, joint=False, **kw)
        res_none = transfer_recording(ldm, content, style, **kw)
    assert res3.N == 3 and torch.equal(res3.windows_out, direct)
    assert bool(torch.isfinite(res3.windows_out).all()) and bool(torch.isfinite(res3.audio).all())
    assert torch.equal(res2.windows_out[:2], pair) and torch.equal(res2.windows_out[2:], last)
    assert not torch.equal(res2.windows_out[1], direct[1]) and not torch.equal(res2.windows_out[2], direct[2])
    assert bool(torch.isfinite(res2.windows_out).all())
    assert torch.equal(res_off.windows_out, res_none.windows_out) and torch.equal(res_off.audio, res_none.audio)
    assert not torch.equal(res3.windows_out, res_none.windows_out)
    # (printed only, the weights are untrained: what the crossfade has to reconcile over each overlap)
    gj, gn = seam_db_gap(res3.windows_out, res3.ref_db, 32), seam_db_gap(res_none.windows_out, res_none.ref_db, 32)
    print("mean |dB| between the two decoded windows over each overlap: joint " + ", ".join(f"{v:.3f}" for v in gj) +
          "; not joint " + ", ".join(f"{v:.3f}" for v in gn))
