"""GPU: the reverse loop's options composed (style mix, guidance, regional keep, style map; the joint loop's seams),
through the public entry points only, on the step-kernel engine at the canonical 16 x 64 latent, 3 steps, both solvers.
Every assertion is bitwise: a captured loop against the eager one, a split batch against the whole one, and a replay
after the set_* methods against a fresh eager call.  No yardstick: each option has its own float64 test."""
import pytest
import torch

pytestmark = pytest.mark.gpu
STEPS, B, H, W, R = 3, 4, 16, 64, 2
SOLVERS = ["ddim", "msolver"]


@pytest.fixture(scope="module")
def ctx(cuda):
    """The model (never modified), its engine and each solver's tables."""
    import models.model as M
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    tt = torch.linspace(99, 0, STEPS + 1).long()
    fd = ldm.noise_scheduler
    coef = {"ddim": fd.reverse_coefs(tt).to(cuda), "msolver": fd.multistep_coefs(tt).to(cuda)}
    return dict(eng=M.engine_for(ldm.unet), coef=coef, keep_coefs=fd.keep_coefs(tt, True), tt=tt, cache={})


def operands(cuda, seed, b=B, composed=True):
    """The state and every option's operands on the device: R stacked references with key biases, a base of the same
    shape, per-sample strengths, a keep with a mask that differs per sample, and a style map's biases."""
    g = torch.Generator().manual_seed(seed)
    r = R if composed else 1
    rand, randn = (lambda *s: torch.rand(*s, generator=g).to(cuda)), (lambda *s: torch.randn(*s, generator=g).to(cuda))
    d = dict(x=randn(b, 32, H, W), s5=rand(b, 256, r * H // 4, W // 4), s6=rand(b, 512, r * H // 8, W // 8),
             z0=randn(b, 32, H, W), n0=randn(b, 32, H, W), w=(rand(b, H, W) > 0.5).float())
    d["w"][0, :, 5:23] = 0.25       # a soft band that is not aligned to a wave's 16 columns
    if composed:
        d.update(kb5=randn(b, r * H * W // 16), kb6=randn(b, r * H * W // 64), s5b=rand(*d["s5"].shape),
                 s6b=rand(*d["s6"].shape), scale=torch.tensor([3.0, -1.25, 0.5, 1.0][:b]),
                 rb5=randn(b, H * W // 16, r), rb6=randn(b, H * W // 64, r))
    return d


def options(ctx, d):
    """The loops' option keywords for the operands d."""
    kw = dict(keep=dict(z0=d["z0"], n0=d["n0"], w=d["w"], coefs=ctx["keep_coefs"]))
    if "kb5" in d:
        kw.update(key_bias5=d["kb5"], key_bias6=d["kb6"], base=(d["s5b"], d["s6b"], None, None), guidance_scale=d["scale"],
                  ref_bias5=d["rb5"], ref_bias6=d["rb6"])
    return kw


def t_table(ctx, cuda, b):
    return ctx["tt"][:-1].view(STEPS, 1).expand(STEPS, b).contiguous().to(cuda)


def eager(ctx, cuda, solver, d, **kw):
    """One eager loop on the operands d; (x, x0_logs, eps_logs)."""
    b = d["x"].shape[0]
    x = d["x"].clone()
    x0l = torch.full((STEPS,) + tuple(x.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    kw = dict(options(ctx, d), **kw)
    with torch.no_grad():
        if solver == "ddim":
            ctx["eng"].ddim_loop(x, d["s5"], d["s6"], t_table(ctx, cuda, b), ctx["coef"][solver], 0.0, x0l, epl, **kw)
        else:
            ctx["eng"].msolver_loop(x, d["s5"], d["s6"], t_table(ctx, cuda, b), ctx["coef"][solver], x0l, epl, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(x0l).all()) and bool(torch.isfinite(epl).all())
    return x, x0l, epl


def composed(ctx, cuda, solver):
    """The composed eager loop at B = 4, once per solver; shared, never modified."""
    if solver not in ctx["cache"]:
        d = operands(cuda, 31)
        ctx["cache"][solver] = (d, eager(ctx, cuda, solver, d))
    return ctx["cache"][solver]


def graphed(ctx, cuda, solver, d, **kw):
    from ldm_amd.engine import GraphedDDIM
    with torch.no_grad():
        return GraphedDDIM(ctx["eng"], d["x"], d["s5"], d["s6"], t_table(ctx, cuda, d["x"].shape[0]), ctx["coef"][solver],
                           0.0, logs=True, solver=solver, **dict(options(ctx, d), **kw))


def same(got, want):
    return all(torch.equal(a, b) for a, b in zip(got, want))


def replay(gd):
    with torch.no_grad():
        x = gd.replay().clone()
    torch.cuda.synchronize()
    return x, gd.x0_logs.clone(), gd.eps_logs.clone()


@pytest.mark.parametrize("solver", SOLVERS)
def test_composed_options_differ_from_fewer(ctx, cuda, solver):
    """Every option of the composition acts: leaving one out changes the result."""
    d, want = composed(ctx, cuda, solver)
    assert not torch.equal(eager(ctx, cuda, solver, d, ref_bias5=None, ref_bias6=None)[0], want[0])
    assert not torch.equal(eager(ctx, cuda, solver, d, key_bias5=None, key_bias6=None)[0], want[0])
    assert not torch.equal(eager(ctx, cuda, solver, dict(d, w=torch.zeros_like(d["w"])))[0], want[0])
    assert not torch.equal(eager(ctx, cuda, solver, dict(d, scale=torch.ones(B)))[0], want[0])


@pytest.mark.parametrize("solver", SOLVERS)
def test_captured_loop_is_the_eager_one_bitwise(ctx, cuda, solver):
    d, want = composed(ctx, cuda, solver)
    gd = graphed(ctx, cuda, solver, d)
    assert same(replay(gd), want)
    assert same(replay(gd), want) and gd.prepare_launches == 1     # and again, without a second prepare


@pytest.mark.parametrize("solver", SOLVERS)
def test_split_is_the_whole_batch_per_sample_bitwise(ctx, cuda, solver):
    d, want = composed(ctx, cuda, solver)
    assert same(eager(ctx, cuda, solver, d, split=2), want)
    assert same(replay(graphed(ctx, cuda, solver, d, split=2)), want)


@pytest.mark.parametrize("solver", SOLVERS)
def test_replay_after_the_setters_is_a_fresh_eager_call_bitwise(ctx, cuda, solver):
    d, first = composed(ctx, cuda, solver)
    d2 = operands(cuda, 32)
    new = dict(d, rb5=d2["rb5"], rb6=d2["rb6"], w=d2["w"], scale=torch.tensor([0.0, 2.0, 1.5, -0.5]))
    gd = graphed(ctx, cuda, solver, d)
    assert same(replay(gd), first)
    gd.set_style_map(new["rb5"], new["rb6"])
    gd.set_keep(new["w"])
    gd.set_guidance_scale(new["scale"])
    got = replay(gd)
    assert gd.prepare_launches == 1           # none of the three is a prepare-phase operand
    want = eager(ctx, cuda, solver, new)
    assert same(got, want) and not torch.equal(want[0], first[0])


@pytest.mark.parametrize("solver", SOLVERS)
def test_joint_loop_with_a_keep_captured_is_the_eager_one_bitwise(ctx, cuda, solver):
    d = operands(cuda, 33, b=2, composed=False)
    want = eager(ctx, cuda, solver, d, seam_cols=2)
    assert torch.equal(want[0][0, :, :, W - 2:], want[0][1, :, :, :2])       # the rows agree across their seam
    assert not torch.equal(eager(ctx, cuda, solver, d)[0], want[0])
    assert same(replay(graphed(ctx, cuda, solver, d, seam_cols=2)), want)
