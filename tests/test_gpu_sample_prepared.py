"""The reverse loop in two phases: ldm_sample_prepare (style and time state) and ldm_sample_run (the loop), the
GraphedDDIM that replays the loop alone while nothing the prepare reads has changed.

Every comparison is bitwise on x and both logs: the two phases make the launches ldm_sample makes, in its order, on
the same operands, so nothing may differ.  Shape: B = 2, H = 8, W = 16, 3 steps (more than one block in every step
kernel, a plane that is not the canonical one, both solvers' history)."""
import ctypes
import os
import re

import pytest
import torch

B, C, H, W, STEPS = 2, 32, 8, 16, 3
L2, L1 = (H // 4) * (W // 4), (H // 8) * (W // 8)
CONFIGS = ["plain", "mix", "guided", "keep", "guided-keep"]
# the loop's forms: the step kernels under both values of use_step, the folded loop on conv.hip, the literal loop
SETTINGS = {"step1": dict(step=1), "step2": dict(step=2), "fold": dict(step=0), "unfolded": dict(fold=False)}
CASES = [(c, s) for c in CONFIGS for s in SETTINGS if not (c == "mix" and s == "unfolded")]   # a mix needs the fold
CASE_IDS = [f"{c}-{s}" for c, s in CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(cuda):
    import models.model as M
    from ldm_amd.engine import UNetEngine
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    engines = {k: UNetEngine(ldm.unet, **kw) for k, kw in SETTINGS.items()}
    times = torch.tensor([99, 66, 33, 0])
    return dict(M=M, ldm=ldm, engines=engines, times=times)


def operands(ctx, cuda, config, seed=7, times=None):
    """The loop's operands on the device for one configuration (a dict of tensors; absent options are None)."""
    g = torch.Generator().manual_seed(seed)
    R = 2 if config == "mix" else 1
    fd = ctx["ldm"].noise_scheduler
    times = ctx["times"] if times is None else times

    def maps():
        return (torch.rand(B, 256, R * H // 4, W // 4, generator=g).to(cuda),
                torch.rand(B, 512, R * H // 8, W // 8, generator=g).to(cuda))
    o = dict(z=torch.randn(B, C, H, W, generator=g).to(cuda), kb5=None, kb6=None, base=None, scale=None, keep=None)
    o["s5"], o["s6"] = maps()
    if config == "mix":     # two references at weights 0.7 / 0.3: the log weight of each key's reference
        lw = torch.log(torch.tensor([0.7, 0.3]))
        o["kb5"] = lw.repeat_interleave(L2).expand(B, R * L2).contiguous().to(cuda)
        o["kb6"] = lw.repeat_interleave(L1).expand(B, R * L1).contiguous().to(cuda)
    if config.startswith("guided"):
        o["base"] = maps() + (None, None)
        o["scale"] = torch.tensor([1.5, -0.5]).to(cuda)
    if config.endswith("keep"):
        w = (torch.rand(B, H, W, generator=g) > 0.5).float()
        o["keep"] = (torch.randn(B, C, H, W, generator=g).to(cuda), torch.randn(B, C, H, W, generator=g).to(cuda),
                     w.to(cuda), fd.keep_coefs(times).to(cuda))
    o["t_table"] = times[:-1].view(STEPS, 1).expand(STEPS, B).contiguous().to(cuda)
    o["coef"] = {"ddim": fd.reverse_coefs(times).to(cuda), "msolver": fd.multistep_coefs(times).to(cuda)}
    return o


class CLoop:
    """The C entries on a workspace of the caller's own, with the engine's bound weights."""

    def __init__(self, eng, o, solver, cuda):
        from ldm_amd import _lib as L
        from ldm_amd import ops
        self.L, self.o = L, o
        self.shape = eng.shape(B, C, H, W)
        guided = o["base"] is not None
        self.w = eng._guided_weights(B, C, H, W) if guided else eng.weights(self.shape)
        self.x = o["z"].clone()
        self.x0l = torch.full((STEPS, B, C, H, W), float("nan"), device=cuda)
        self.epl = torch.full_like(self.x0l, float("nan"))
        a = L.SampleArgs(solver=L.SOLVER[solver], nsteps=STEPS, eta=0.0, x=self.x.data_ptr(), s5=o["s5"].data_ptr(),
                         s6=o["s6"].data_ptr(), t_table=o["t_table"].data_ptr(), coef_table=o["coef"][solver].data_ptr(),
                         x0_logs=self.x0l.data_ptr(), eps_logs=self.epl.data_ptr(), stream=ops.stream_handle())
        if o["kb5"] is not None or guided and o["s5"].shape[2] != H // 4:
            a.S5, a.S6 = o["s5"].shape[2] * o["s5"].shape[3], o["s6"].shape[2] * o["s6"].shape[3]
            a.key_bias5, a.key_bias6 = o["kb5"].data_ptr(), o["kb6"].data_ptr()
        if guided:
            a.s5_base, a.s6_base, a.guide_scale = o["base"][0].data_ptr(), o["base"][1].data_ptr(), o["scale"].data_ptr()
        if o["keep"] is not None:
            a.z0, a.n0, a.keep, a.keep_coef = (v.data_ptr() for v in o["keep"])
        n = L.load().ldm_sample_workspace_floats(ctypes.byref(self.shape), ctypes.byref(self.w), ctypes.byref(a))
        assert n > 0
        self.ws = torch.zeros(int(n), device=cuda)
        a.workspace = self.ws.data_ptr()
        self.a = a

    def call(self, entry):
        self.L.call(entry, ctypes.byref(self.shape), ctypes.byref(self.w), ctypes.byref(self.a))

    def poison(self):
        """NaN everywhere in the workspace but in the two counter regions, which stay zero."""
        r = (ctypes.c_int64 * 4)()
        self.L.call("ldm_sample_workspace_zeroed", ctypes.byref(self.shape), ctypes.byref(self.w), ctypes.byref(self.a), r)
        assert all(0 <= r[i] and r[i] + r[i + 1] <= self.ws.numel() for i in (0, 2))
        self.ws.fill_(float("nan"))
        for i in (0, 2):
            self.ws[r[i]:r[i] + r[i + 1]].zero_()

    def result(self):
        torch.cuda.synchronize()
        return self.x.clone(), self.x0l.clone(), self.epl.clone()


def same(got, want, what=""):
    for name, g, w in zip(("x", "x0 logs", "eps logs"), got, want):
        assert bool(torch.isfinite(w).all()), f"{what}{name}: the reference is not finite"
        assert torch.equal(g, w), f"{what}{name}"


def one_shot(ctx, cuda, config, setting, solver, o=None):
    o = operands(ctx, cuda, config) if o is None else o
    ref = CLoop(ctx["engines"][setting], o, solver, cuda)
    ref.call("ldm_sample")
    return o, ref.result()


# ---- 1. prepare then run is ldm_sample -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["ddim", "msolver"])
@pytest.mark.parametrize("config,setting", CASES, ids=CASE_IDS)
def test_prepare_then_run_is_ldm_sample_bitwise(ctx, cuda, config, setting, solver):
    o, want = one_shot(ctx, cuda, config, setting, solver)
    two = CLoop(ctx["engines"][setting], o, solver, cuda)
    two.call("ldm_sample_prepare")
    torch.cuda.synchronize()
    assert torch.equal(two.x, o["z"]), "the prepare phase wrote x"
    assert bool(torch.isnan(two.x0l).all()) and bool(torch.isnan(two.epl).all()), "the prepare phase wrote the logs"
    two.call("ldm_sample_run")
    same(two.result(), want)


# ---- 2. the run phase leaves the prepared state alone ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config,setting", CASES, ids=CASE_IDS)
def test_two_runs_after_one_prepare_on_a_poisoned_workspace(ctx, cuda, config, setting):
    o, want = one_shot(ctx, cuda, config, setting, "ddim")
    two = CLoop(ctx["engines"][setting], o, "ddim", cuda)
    two.poison()
    two.call("ldm_sample_prepare")
    for i in range(2):
        two.x.copy_(o["z"])
        two.x0l.fill_(float("nan"))
        two.epl.fill_(float("nan"))
        two.call("ldm_sample_run")
        same(two.result(), want, f"run {i}: ")


# ---- 3. GraphedDDIM: replay and invalidation -------------------------------------------------------------------------
def graphed(ctx, cuda, o, split=1):
    from ldm_amd.engine import GraphedDDIM
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    with torch.no_grad():
        return GraphedDDIM(eng, o["z"], o["s5"], o["s6"], o["t_table"], o["coef"]["ddim"], 0.0, logs=True, split=split,
                           key_bias5=o["kb5"], key_bias6=o["kb6"])


def replayed(gd):
    gd.replay()
    torch.cuda.synchronize()
    return gd.x.clone(), gd.x0_logs.clone(), gd.eps_logs.clone()


@pytest.mark.gpu
def test_graphed_replays_prepare_once_then_once_per_change(ctx, cuda):
    o, want = one_shot(ctx, cuda, "plain", "step2", "ddim")
    gd = graphed(ctx, cuda, o)
    for i in range(3):
        same(replayed(gd), want, f"replay {i}: ")
    assert gd.prepare_launches == 1
    # a style map written through torch
    other = operands(ctx, cuda, "plain", seed=8)
    gd.s5.copy_(other["s5"])
    o2 = dict(o, s5=other["s5"])
    same(replayed(gd), replayed(graphed(ctx, cuda, o2)), "after s5.copy_: ")
    assert gd.prepare_launches == 2
    same(replayed(gd), one_shot(ctx, cuda, "plain", "step2", "ddim", o2)[1], "after s5.copy_, second replay: ")
    assert gd.prepare_launches == 2
    # the t table
    o3 = dict(o2, t_table=(o["t_table"] - 7).contiguous())
    gd.t_table.copy_(o3["t_table"])
    same(replayed(gd), replayed(graphed(ctx, cuda, o3)), "after t_table.copy_: ")
    assert gd.prepare_launches == 3
    # a raw-pointer write moves no version: the replay is stale until invalidate()
    stale = replayed(gd)
    v = gd.s6._version
    gd.s6.data.copy_(other["s6"])
    assert gd.s6._version == v
    same(replayed(gd), stale, "raw write, no invalidate: ")
    assert gd.prepare_launches == 3
    gd.invalidate()
    o4 = dict(o3, s6=other["s6"])
    same(replayed(gd), replayed(graphed(ctx, cuda, o4)), "after invalidate(): ")
    assert gd.prepare_launches == 4
    # what the run phase reads needs no prepare
    gd.x_init.copy_(other["z"])
    same(replayed(gd), one_shot(ctx, cuda, "plain", "step2", "ddim", dict(o4, z=other["z"]))[1], "after x_init.copy_: ")
    assert gd.prepare_launches == 4


@pytest.mark.gpu
def test_graphed_sees_a_key_bias_written_through_torch(ctx, cuda):
    o = operands(ctx, cuda, "mix")
    gd = graphed(ctx, cuda, o)
    same(replayed(gd), one_shot(ctx, cuda, "mix", "step2", "ddim", o)[1])
    lw = torch.log(torch.tensor([0.2, 0.8]))
    kb5 = lw.repeat_interleave(L2).expand(B, 2 * L2).contiguous().to(cuda)
    gd.kb5.copy_(kb5)
    same(replayed(gd), replayed(graphed(ctx, cuda, dict(o, kb5=kb5))), "after kb5.copy_: ")
    assert gd.prepare_launches == 2


@pytest.mark.gpu
def test_graphed_sees_a_weight_written_through_torch(ctx, cuda):
    """in_proj_weight of CA1: the prepare reads it raw (the key fold) and packed (the K/V projection), and the loop
    reads the enc4 / bottleneck folds made from it, so a replay that kept any stale copy would differ."""
    o = operands(ctx, cuda, "plain")
    gd = graphed(ctx, cuda, o)
    before = replayed(gd)
    p = ctx["ldm"].unet.cross_attention1.multihead_attn.in_proj_weight
    saved = p.detach().clone()
    try:
        with torch.no_grad():
            p.mul_(1.25)
        got = replayed(gd)
        assert gd.prepare_launches == 2
        same(got, replayed(graphed(ctx, cuda, o)), "after the weight change: ")
        assert not torch.equal(got[0], before[0])
    finally:
        with torch.no_grad():
            p.copy_(saved)


@pytest.mark.gpu
def test_graphed_split_chains_follow_a_style_change(ctx, cuda):
    o = operands(ctx, cuda, "plain")
    other = operands(ctx, cuda, "plain", seed=8)
    gd = graphed(ctx, cuda, o, split=2)
    first = replayed(gd)
    same(replayed(gd), first, "second replay: ")
    assert gd.prepare_launches == 1
    o2 = dict(o, s5=other["s5"], t_table=(o["t_table"] - 7).contiguous())
    gd.s5.copy_(other["s5"])
    gd.t_table.copy_(o2["t_table"])     # (gd.t_table may be o's own tensor: a device table is not cloned)
    same(replayed(gd), replayed(graphed(ctx, cuda, o2, split=2)), "after the change: ")
    assert gd.prepare_launches == 2


# ---- 4. nothing else writes a captured loop's prepared state -----------------------------------------------------------
@pytest.mark.gpu
def test_graphed_state_survives_other_work_on_the_engine(ctx, cuda):
    """The engine's shared workspaces are written by forward() (its K/V projections land where a loop's do), by the
    eager loops and by the replays of a caller's captured forward; a GraphedDDIM prepares on workspaces of its own, so
    a replay that skips the prepare graph after any of them still equals the one-shot call.  The eager loops
    themselves prepare on every call."""
    from ldm_amd.graphs import capture
    o, want = one_shot(ctx, cuda, "plain", "step2", "ddim")
    other = operands(ctx, cuda, "plain", seed=8)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    gd = graphed(ctx, cuda, o)
    same(replayed(gd), want, "first replay: ")
    y = torch.empty_like(o["z"])
    with torch.no_grad():
        eng.forward(o["z"], o["t_table"][0], other["s5"], other["s6"], out=y)      # warm-up, then captured
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g):
            eng.forward(o["z"], o["t_table"][0], other["s5"], other["s6"], out=y)

        def eager(s5, s6):
            x = o["z"].clone()
            x0l = torch.empty((STEPS, B, C, H, W), device=cuda)
            epl = torch.empty_like(x0l)
            eng.ddim_loop(x, s5, s6, o["t_table"], o["coef"]["ddim"], 0.0, x0l, epl)
            torch.cuda.synchronize()
            return x, x0l, epl

        same(eager(o["s5"], o["s6"]), want, "eager loop: ")
        g.replay()                                  # rewrites the shared workspace's K/V projections with another style
        same(eager(o["s5"], o["s6"]), want, "eager loop, same tensors, after a captured forward's replay: ")
        eager(other["s5"], other["s6"])
    same(replayed(gd), want, "replay after the other work: ")
    assert gd.prepare_launches == 1


# ---- 5. host only ----------------------------------------------------------------------------------------------------
def test_prepared_key_follows_versions():
    from ldm_amd.engine import prepared_key
    a, b, t = torch.zeros(2, 3), torch.zeros(4), torch.zeros(3, 2, dtype=torch.int64)
    ops_ = (a, b, None, t)
    k0 = prepared_key(ops_, (1, 2, 3))
    assert prepared_key(ops_, (1, 2, 3)) == k0
    assert prepared_key(ops_, (1, 2, 4)) != k0, "a new weight version"
    assert prepared_key(ops_, (1, 2, 3), (5,)) != prepared_key(ops_, (1, 2, 3), (6,))
    assert prepared_key((a, None, b, t), (1, 2, 3)) != k0, "operands are positional"
    assert prepared_key((a[:1], b, None, t), (1, 2, 3)) != k0, "another shape at the same address"
    b.copy_(torch.ones(4))
    k1 = prepared_key(ops_, (1, 2, 3))
    assert k1 != k0, "an in-place write through torch"
    t.add_(1)
    assert prepared_key(ops_, (1, 2, 3)) != k1
    v = a._version
    a.data.fill_(1.0)       # .data has a version counter of its own: the key cannot see this write
    assert a._version == v


def test_prepare_and_run_are_declared_and_exported():
    from ldm_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldm_capi.h")).read()
    lib = _lib.load()
    for name in ("ldm_sample_prepare", "ldm_sample_run", "ldm_sample_workspace_zeroed"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in ldm_capi.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
