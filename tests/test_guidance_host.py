"""CPU: style guidance's host-side rules and its float64 yardstick (tests/guidance_ref.py).

The validation errors of the guidance arguments are raised before anything touches a device; scale 1 without a base
reaches the unguided engine call, argument for argument (a stub engine records it); the yardstick reduces to the plain
float64 loop at s = 1 and to the base-only loop at s = 0."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as GR      # noqa: E402
import solver_ref as SR        # noqa: E402


def emb(B=2, H=16, W=16, seed=0, R=1):
    g = torch.Generator().manual_seed(seed)
    return {"s5": torch.rand(B, 256, R * H // 4, W // 4, generator=g), "s6": torch.rand(B, 512, R * H // 8, W // 8, generator=g)}


@pytest.fixture(scope="module")
def ldm():
    import models.model as M
    torch.manual_seed(0)
    return M.LDM(32, pretrained_path="").eval()


def test_scale_validation(ldm):
    from ldm_amd.engine import UNetEngine
    z = torch.zeros(2, 32, 16, 16)
    for bad in (float("nan"), float("inf"), -float("inf"), torch.tensor([1.0, float("nan")])):
        with pytest.raises(ValueError, match="finite"):
            ldm.style_conditioned_sample(z, emb(), steps=2, t_start=9, guidance_scale=bad, base_embedding=emb(seed=1))
        with pytest.raises(ValueError, match="finite"):
            UNetEngine.guidance_scale(bad, 2)
    with pytest.raises(ValueError, match="per sample"):
        UNetEngine.guidance_scale(torch.ones(3), 2)
    s = UNetEngine.guidance_scale(-1.25, 3)
    assert s.dtype == torch.float32 and s.tolist() == [-1.25] * 3 and s.is_contiguous()
    s = UNetEngine.guidance_scale(torch.tensor([3.7, -1.25], dtype=torch.float64), 2)
    assert s.dtype == torch.float32 and torch.equal(s, torch.tensor([3.7, -1.25]))


def test_scale_without_a_base_raises(ldm):
    z = torch.zeros(2, 32, 16, 16)
    with pytest.raises(ValueError, match="base"):
        ldm.style_conditioned_sample(z, emb(), steps=2, t_start=9, guidance_scale=2.0)
    with pytest.raises(ValueError, match="base"):
        ldm.style_conditioned_sample(z, emb(), steps=2, t_start=9, guidance_scale=torch.tensor([1.0, 1.5]))


def test_base_key_counts_must_match(ldm):
    z = torch.zeros(2, 32, 16, 16)
    with pytest.raises(ValueError) as ei:
        ldm.style_conditioned_sample(z, emb(R=2), steps=2, t_start=9, guidance_scale=2.0, base_embedding=emb(seed=1))
    msg = str(ei.value)
    assert "(2, 256, 8, 4)" in msg and "(2, 256, 4, 4)" in msg      # both shapes are named


def test_tile_embedding_shapes(ldm):
    import models.model as M
    e = emb(seed=3)
    t = M.LDM.tile_embedding(e, 3)
    assert tuple(t["s5"].shape) == (2, 256, 12, 4) and tuple(t["s6"].shape) == (2, 512, 6, 2)
    assert t["key_bias5"] is None and t["key_bias6"] is None and t["refs"] == 3
    for r in range(3):          # reference r owns the rows [r*h, (r+1)*h)
        assert torch.equal(t["s5"][:, :, 4 * r:4 * r + 4], e["s5"]) and torch.equal(t["s6"][:, :, 2 * r:2 * r + 2], e["s6"])
    assert M.LDM.tile_embedding(e, 1)["s5"] is e["s5"]
    with pytest.raises(ValueError):
        M.LDM.tile_embedding(e, 0)
    with pytest.raises(ValueError):
        M.LDM.tile_embedding(dict(e, key_bias5=torch.zeros(2, 16)), 2)


def test_signature_table_has_the_new_entries():
    from ldm_amd import _lib
    for n in ("ldm_sample", "ldm_sample_workspace_floats", "ldm_guide_eps"):
        assert n in _lib.SIGNATURES
    # two base maps, two base biases and the scale beside the mix fields; the regional keep's four operands
    fields = [f[0] for f in _lib.SampleArgs._fields_]
    for f in ("S5", "S6", "key_bias5", "key_bias6", "s5_base", "s6_base", "key_bias5_base", "key_bias6_base",
              "guide_scale", "z0", "n0", "keep", "keep_coef"):
        assert fields.count(f) == 1
    assert len(_lib.SIGNATURES["ldm_guide_eps"][1]) == 7


class StubEngine:
    """Records the loop calls LDM._reverse makes (no device work)."""

    def __init__(self):
        self.calls = []

    def ddim_loop(self, *a, **kw):
        self.calls.append(("ddim_loop", len(a), dict(kw)))

    def msolver_loop(self, *a, **kw):
        self.calls.append(("msolver_loop", len(a), dict(kw)))


@pytest.mark.parametrize("solver,name,nargs", [("dpmpp2m", "msolver_loop", 7), ("ddim", "ddim_loop", 8)])
def test_scale_one_without_a_base_is_the_unguided_call(ldm, monkeypatch, solver, name, nargs):
    import models.model as M
    stub = StubEngine()
    monkeypatch.setattr(M, "engine_for", lambda unet: stub)
    monkeypatch.setattr(M.ops, "f32c", lambda t: t.float().contiguous())
    z = torch.zeros(2, 32, 16, 16)
    for kw in ({}, {"guidance_scale": 1.0}, {"guidance_scale": torch.ones(2)}, {"guidance_scale": 1, "base_embedding": None}):
        ldm.style_conditioned_sample(z, emb(), steps=2, t_start=9, solver=solver, **kw)
    assert len(stub.calls) == 4
    for c in stub.calls:        # today's call: positional operands only, no key bias, no guidance keywords
        assert c == (name, nargs, {})
    # with a base the guided keywords arrive, scale as an fp32 [B] tensor
    stub.calls.clear()
    ldm.style_conditioned_sample(z, emb(), steps=2, t_start=9, solver=solver, guidance_scale=1.0, base_embedding=emb(seed=1))
    ldm.style_conditioned_sample(z, emb(), steps=2, t_start=9, solver=solver, guidance_scale=2.5, base_embedding=emb(seed=1))
    assert [c[0] for c in stub.calls] == [name, name]
    for c, want in zip(stub.calls, (1.0, 2.5)):
        assert set(c[2]) == {"key_bias5", "key_bias6", "base", "guidance_scale"}
        assert c[2]["guidance_scale"].tolist() == [want, want] and len(c[2]["base"]) == 4


def test_engine_entry_points_refuse_a_scale_without_a_base():
    from ldm_amd.engine import UNetEngine
    assert UNetEngine.is_unguided(None, 1.0) and UNetEngine.is_unguided(None, torch.ones(3))
    assert not UNetEngine.is_unguided(None, 1.5) and not UNetEngine.is_unguided(None, torch.tensor([1.0, 0.0]))
    assert not UNetEngine.is_unguided((None,) * 4, 1.0)


def test_cli_parsing():
    from models.transfer import parse_args
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "--out", "o.wav"])
    assert a.guidance_scale == 1.0 and a.base_style is None
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "--solver", "dpmpp2m", "--guidance-scale", "2.5", "--out", "o.wav"])
    assert a.guidance_scale == 2.5 and a.base_style is None
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "--solver", "dpmpp2m", "--guidance-scale", "0.5",
                    "--base-style", "c.wav", "--out", "o.wav"])
    assert a.base_style == "c.wav"
    with pytest.raises(SystemExit):
        parse_args(["--content", "a.wav", "--style", "b.wav", "--guidance-scale", "nan", "--out", "o.wav"])


# ---- the yardstick --------------------------------------------------------------------------------------------------
def lin_eps(k):
    return lambda x, i: k * x + 0.01 * (i + 1)


@pytest.mark.parametrize("solver,eta", [("dpmpp2m", 0.0), ("dpmpp1", 0.0), ("ddim", 0.0), ("ddim", 1.0)])
def test_yardstick_reduces_to_the_plain_loops(solver, eta):
    ab = SR.alpha_bar(200)
    times = SR.sample_times(99, 4)
    x = np.linspace(-2.0, 2.0, 2 * 3 * 5).reshape(2, 3, 5)
    et, eb = lin_eps(0.3), lin_eps(-0.2)
    want_t = GR.plain(ab, times, x, et, solver, eta)
    want_b = GR.plain(ab, times, x, eb, solver, eta)
    g1 = GR.solve(ab, times, x, et, eb, 1.0, solver, eta)
    g0 = GR.solve(ab, times, x, et, eb, 0.0, solver, eta)
    assert rel_err(g1[0], want_t[0]) < 1e-14 and rel_err(np.stack(g1[1]), np.stack(want_t[1])) < 1e-14
    assert rel_err(g0[0], want_b[0]) == 0.0 and rel_err(np.stack(g0[2]), np.stack(want_b[2])) == 0.0
    # one strength per sample: each sample follows its own loop
    gp = GR.solve(ab, times, x, et, eb, np.array([1.0, 0.0]), solver, eta)
    assert rel_err(gp[0][0], want_t[0][0]) < 1e-14 and rel_err(gp[0][1], want_b[0][1]) == 0.0
    # target == base: the strength drops out
    gs = GR.solve(ab, times, x, et, et, np.array([3.7, -1.25]), solver, eta)
    assert rel_err(gs[0], want_t[0]) == 0.0
    # and it is an extrapolation, not a blend of end points: s = 3 differs from both
    g3 = GR.solve(ab, times, x, et, eb, 3.0, solver, eta)
    assert rel_err(g3[0], want_t[0]) > 1e-3 and rel_err(g3[0], want_b[0]) > 1e-3


def test_yardstick_ddim_step_is_the_oracles():
    from oracle import ldm_torch_cpu as TC
    ab = SR.alpha_bar(200)
    times = SR.sample_times(99, 4)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64)
    e = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64)
    for eta in (0.0, 1.0):
        t = torch.full((2,), int(times[1]), dtype=torch.long)
        tn = torch.full((2,), int(times[2]), dtype=torch.long)
        want, want0 = TC.ddim_step(torch.from_numpy(ab), x, e, t, tn, eta)
        got, got0 = GR.ddim_step(ab, times, 1, x.numpy(), e.numpy(), eta)
        assert rel_err(got, want.numpy()) < 1e-13 and rel_err(got0, want0.numpy()) < 1e-13
