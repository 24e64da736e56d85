"""Gradient-norm clipping and EMA weights inside the optimizer's launches.

1. ldm_unscale_check_norm + ldm_grad_norm_finalize against the float64 reference (clip_ema_ref): norm and
   coefficient within 1 fp32 ulp (the kernel's squares are exact and its sums fp64; only the summation order
   differs from numpy's, so the one final cast moves by at most one ulp); bitwise repeatable partials; the
   unscaled gradients and found_inf bitwise those of ldm_unscale_check.
2. Fused equals unfused, bitwise: clip_grad_norm_ in place + plain step() + ldm_ema_update against one _ext launch
   with the same coefficient and the EMA (Adam, AdamW, Adam with weight decay; host-step and capturable forms).
3. Parity with CPU torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW + a float64 EMA: rel_err < 1e-6,
   the bound test_adam_matches_torch uses for the same kernels.
4. Off means off: an _ext call with an all-NULL record is bitwise ldm_adam_step; a trainer with both options None
   is bitwise a trainer built without them and calls no new entry point.
5. Scaler interplay: an inf gradient skips parameters, moments, EMA and step count and backs the scale off; the
   following clean step is clipped and applied.
6. Trainer, eager and graphed: bitwise equal parameters, EMA and last_grad_norm; ema_weights() swaps and restores;
   the optimizer's state dict carries the EMA.

The tensor set (clip_ema_ref.SHAPES) reaches every path of the chunk map and of chunk_for in one table.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import clip_ema_ref as R
import recipe
from conftest import rel_err

pytestmark = pytest.mark.gpu

CHUNK = 4096
KINDS = ("adam", "adam_wd", "adamw")
NCHUNKS = sum((int(np.prod(s)) + CHUNK - 1) // CHUNK for s in R.SHAPES)


def _place(arrs, cuda):
    """The arrays on the device; the one at OFFSET_INDEX as a contiguous view one element into its storage."""
    out = []
    for i, a in enumerate(arrs):
        t = torch.from_numpy(a)
        if i == R.OFFSET_INDEX:
            base = torch.empty(t.numel() + 1, dtype=torch.float32, device=cuda)
            base[1:].copy_(t.reshape(-1))
            v = base[1:].view(t.shape)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4
            out.append(v)
        else:
            out.append(t.to(cuda))
    return out


def _params(cuda, seed=10):
    return [torch.nn.Parameter(t) for t in _place(R.tensors(seed), cuda)]


def _set_grads(ps, arrs, cuda, factor=1.0):
    for p, g in zip(ps, _place(arrs, cuda)):
        p.grad = g.mul_(factor) if factor != 1.0 else g      # (in place: the offset view stays one)


def _table(hoptim, gs):
    return hoptim._SlotTable(gs, gs, [None] * len(gs), [None] * len(gs))


def _stream():
    from ldm_amd.ops import stream_handle
    return stream_handle()


# ---- 1. norm ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def norm_case():
    gs = R.grads(21)
    return gs, R.grad_norm(gs)


def _norm_run(cuda, gs_np, max_norm):
    from ldm_amd import _lib as L
    from ldm_amd import optim as hoptim
    gs = [g.mul_(1024.0) for g in _place(gs_np, cuda)]      # scaled by a power of two: the unscale is exact
    assert gs[R.OFFSET_INDEX].data_ptr() % 16 == 4
    tab = _table(hoptim, gs)
    assert tab.nchunks == NCHUNKS
    inv = torch.full((1,), 1.0 / 1024.0, device=cuda)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    partials = torch.full((tab.nchunks,), -1.0, dtype=torch.float64, device=cuda)
    out = torch.full((2,), -1.0, device=cuda)
    L.call("ldm_unscale_check_norm", tab.slots.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_start.data_ptr(),
           tab.nchunks, CHUNK, inv.data_ptr(), bad.data_ptr(), partials.data_ptr(), _stream())
    L.call("ldm_grad_norm_finalize", partials.data_ptr(), tab.nchunks, float(max_norm), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return gs, bad, partials, out


@pytest.mark.parametrize("max_norm", [1.0, 1e6, 0.0, -1.0])
def test_norm_and_coefficient_within_one_ulp(cuda, norm_case, max_norm):
    gs_np, norm = norm_case
    assert 100.0 < norm < 1e4
    _, bad, partials, out = _norm_run(cuda, gs_np, max_norm)
    coef = R.clip_coef(norm, max_norm)
    got_norm, got_coef = (np.float32(v) for v in out.cpu().numpy())
    print(f"max_norm {max_norm}: norm {got_norm!r} (ref {np.float32(norm)!r}), coef {got_coef!r} (ref {np.float32(coef)!r})")
    assert int(bad.item()) == 0
    assert R.ulp_distance(got_norm, np.float32(norm)) <= 1
    assert R.ulp_distance(got_coef, np.float32(coef)) <= 1
    if max_norm == 1.0:
        assert got_coef < 1.0
    else:
        assert got_coef == 1.0          # the norm below max_norm, or norm only: exactly 1
    # each partial is its chunk's sum of squares (fp64 sums of exact squares: 1e-12 covers any order)
    flat = np.concatenate([np.pad(g.reshape(-1).astype(np.float64) ** 2, (0, -g.size % CHUNK)).reshape(-1, CHUNK).sum(1)
                           for g in gs_np])
    assert rel_err(partials.cpu().numpy(), flat) < 1e-12


def test_norm_pass_is_repeatable_and_unscales_like_unscale_check(cuda, norm_case):
    from ldm_amd import _lib as L
    from ldm_amd import optim as hoptim
    gs_np, _ = norm_case
    g1, bad1, part1, out1 = _norm_run(cuda, gs_np, 1.0)
    g2, bad2, part2, out2 = _norm_run(cuda, gs_np, 1.0)
    assert torch.equal(part1, part2) and torch.equal(out1, out2)
    # ldm_unscale_check on the same input
    g3 = [g.mul_(1024.0) for g in _place(gs_np, cuda)]
    tab = _table(hoptim, g3)
    inv = torch.full((1,), 1.0 / 1024.0, device=cuda)
    bad3 = torch.zeros(1, dtype=torch.int32, device=cuda)
    L.call("ldm_unscale_check", tab.slots.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_start.data_ptr(),
           tab.nchunks, CHUNK, inv.data_ptr(), bad3.data_ptr(), _stream())
    torch.cuda.synchronize()
    for a, b, ref in zip(g1, g3, gs_np):
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), ref)
    assert torch.equal(bad1, bad3)


def test_norm_pass_flags_non_finite_like_unscale_check(cuda, norm_case):
    gs_np = [g.copy() for g in norm_case[0]]
    gs_np[3][4096] = np.inf                              # the one-element tail chunk of the 4097 tensor
    _, bad, partials, out = _norm_run(cuda, gs_np, 1.0)
    assert int(bad.item()) == 1
    norm, coef = out.cpu().numpy()
    assert np.isinf(norm) and coef == 0.0                # torch: max_norm / (inf + 1e-6) = 0
    gs_np[3][4096] = np.nan
    _, bad, partials, out = _norm_run(cuda, gs_np, 1.0)
    norm, coef = out.cpu().numpy()
    assert int(bad.item()) == 1 and np.isnan(norm) and np.isnan(coef)


# ---- 2. / 3. fused, unfused, torch ---------------------------------------------------------------------------
def _make_opt(hoptim, kind, ps, capturable=False, lr=5e-3):
    if kind == "adam":
        return hoptim.Adam(ps, lr=lr, capturable=capturable)
    if kind == "adam_wd":
        return hoptim.Adam(ps, lr=lr, weight_decay=0.01, capturable=capturable)
    return hoptim.AdamW(ps, lr=lr, capturable=capturable)


MAX_NORM, DECAY = 1.0, 0.9


@pytest.fixture(scope="module")
def fused_runs(cuda):
    """{(kind, capturable): (params, optimizer)} after three fused steps (one _ext launch per step)."""
    from ldm_amd import optim as hoptim
    runs = {}
    for kind in KINDS:
        for cap in (False, True):
            ps = _params(cuda)
            opt = _make_opt(hoptim, kind, ps, cap)
            opt.attach_ema(DECAY)
            for step in range(3):
                _set_grads(ps, R.grads(100 + step), cuda)
                pair = hoptim.grad_norm_coef(ps, MAX_NORM)
                opt.step(grad_mul=pair[1:2])
            torch.cuda.synchronize()
            runs[(kind, cap)] = (ps, opt)
    return runs


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_equals_unfused_bitwise(cuda, fused_runs, kind, capturable):
    from ldm_amd import optim as hoptim
    ps = _params(cuda)
    assert ps[R.OFFSET_INDEX].data_ptr() % 16 == 4
    opt = _make_opt(hoptim, kind, ps, capturable)
    emas = [p.detach().clone() for p in ps]
    for step in range(3):
        _set_grads(ps, R.grads(100 + step), cuda)
        norm = hoptim.clip_grad_norm_(ps, MAX_NORM)
        assert norm.dim() == 0 and norm.device.type == "cuda" and float(norm) > MAX_NORM
        opt.step()
        hoptim.ema_update_(emas, [p.detach() for p in ps], DECAY)
    torch.cuda.synchronize()
    fps, fopt = fused_runs[(kind, capturable)]
    for p, e, fp in zip(ps, emas, fps):
        assert torch.equal(p.detach(), fp.detach())
        assert torch.equal(opt.state[p]["exp_avg"], fopt.state[fp]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], fopt.state[fp]["exp_avg_sq"])
        assert torch.equal(e, fopt.state[fp]["ema"])
        assert not torch.equal(e, p.detach()) or p.numel() == 0
        assert float(opt.state[p]["step"]) == float(fopt.state[fp]["step"]) == 3.0


@pytest.mark.parametrize("kind", KINDS)
def test_clipped_step_and_ema_match_torch(cuda, fused_runs, kind):
    ps_ref = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in R.tensors(10)]
    kw = dict(lr=5e-3)
    if kind == "adam":
        ref = torch.optim.Adam(ps_ref, **kw)
    elif kind == "adam_wd":
        ref = torch.optim.Adam(ps_ref, weight_decay=0.01, **kw)
    else:
        ref = torch.optim.AdamW(ps_ref, **kw)
    emas = [p.detach().double().clone() for p in ps_ref]
    for step in range(3):
        for p, g in zip(ps_ref, R.grads(100 + step)):
            p.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_(ps_ref, MAX_NORM)
        ref.step()
        emas = [e + (1.0 - DECAY) * (p.detach().double() - e) for e, p in zip(emas, ps_ref)]
    for cap in (False, True):
        fps, fopt = fused_runs[(kind, cap)]
        for a, e, b in zip(ps_ref, emas, fps):
            ep = rel_err(b.detach().double().cpu().numpy(), a.detach().double().numpy())
            ee = rel_err(fopt.state[b]["ema"].double().cpu().numpy(), e.numpy())
            assert ep < 1e-6 and ee < 1e-6, (kind, cap, tuple(a.shape), ep, ee)


def test_fused_step_matches_float64_reference(cuda, fused_runs):
    """The same three clipped AdamW steps and the EMA in numpy float64 (clip_ema_ref): 1e-6 as above."""
    ps = R.tensors(10)
    ms = [np.zeros(p.shape) for p in ps]
    vs = [np.zeros(p.shape) for p in ps]
    es = [p.astype(np.float64) for p in ps]
    ps = [p.astype(np.float64) for p in ps]
    for step in range(3):
        gs = R.grads(100 + step)
        coef = R.clip_coef(R.grad_norm(gs), MAX_NORM)
        assert coef < 1.0
        for i, g in enumerate(gs):
            ps[i], ms[i], vs[i] = R.adam_step(ps[i], g, ms[i], vs[i], step + 1, 5e-3, weight_decay=1e-2,
                                              decoupled=True, coef=coef)
            es[i] = R.ema_step(es[i], ps[i], DECAY)
    fps, fopt = fused_runs[("adamw", False)]
    for p, e, fp in zip(ps, es, fps):
        assert rel_err(fp.detach().double().cpu().numpy(), p) < 1e-6
        assert rel_err(fopt.state[fp]["ema"].double().cpu().numpy(), e) < 1e-6


# ---- 4. off means off -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev, record", [pytest.param(False, "null", id="null"), pytest.param(False, "empty", id="empty"),
                                         pytest.param(True, "null", id="dev-null"),
                                         pytest.param(True, "empty", id="dev-empty")])
def test_ext_entry_with_nothing_set_is_the_plain_step(cuda, dev, record):
    """ldm_adam_step against ldm_adam_step_ext, and (dev) the capturable pair ldm_adam_step_dev against
    ldm_adam_step_dev_ext from a device step count of 6, with a null and with an empty record."""
    from ldm_amd import _lib as L
    from ldm_amd import optim as hoptim
    res = []
    for ext in (False, True):
        ps = [p.detach() for p in _params(cuda)]
        gs = _place(R.grads(300), cuda)
        ms = [torch.from_numpy(a).to(cuda) for a in R.tensors(301, 1e-2)]
        vs = [torch.from_numpy(np.abs(a)).to(cuda) for a in R.tensors(302, 1e-4)]
        tab = hoptim._SlotTable(ps, gs, ms, vs)
        step = torch.full((), 6.0, dtype=torch.float32, device=cuda)
        scalars = torch.zeros(8, dtype=torch.float32, device=cuda)
        args = (tab.slots.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_start.data_ptr(), tab.nchunks, CHUNK,
                1e-3, 0.9, 0.999, 1e-8, 0.01, 0)
        args += (step.data_ptr(), None, scalars.data_ptr()) if dev else (7, None)
        name = "ldm_adam_step_dev" if dev else "ldm_adam_step"
        if not ext:
            L.call(name, *args, _stream())
        else:
            rec = L.AdamExt(None, None, 0.0)
            L.call(name + "_ext", *args, None if record == "null" else ctypes.byref(rec), _stream())
        torch.cuda.synchronize()
        res.append((ps, ms, vs, [step]))
    assert float(res[0][3][0]) == (7.0 if dev else 6.0)
    for a, b in zip(res[0], res[1]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


class _ZeroFeat(torch.nn.Module):
    def forward(self, a, b):
        return torch.zeros((), device=a.device)


def _model(cuda):
    import models.model as M
    m = M.LDM(32, pretrained_path="")
    recipe.fill_module(m, seed=700)
    m.feature_loss_net = _ZeroFeat()
    return m.to(cuda).train()


def _inputs(cuda, seed):
    content = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), seed)).to(cuda)
    style = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), seed + 1)).to(cuda)
    t = torch.tensor([20, 120], device=cuda)
    noise = torch.from_numpy(recipe.normal((2, 32, 16, 16), seed + 2)).to(cuda)
    return content, style, t, noise


def test_trainer_with_both_options_off_is_the_old_trainer(cuda, monkeypatch):
    import models.train as TR
    from ldm_amd import _lib as L
    called = set()
    real = L.call

    def spy(name, *a):
        called.add(name)
        return real(name, *a)

    monkeypatch.setattr(L, "call", spy)
    inp = _inputs(cuda, 910)
    sds = []
    for kw in ({}, dict(max_grad_norm=None, ema_decay=None)):
        tr = TR.LDMTrainer(_model(cuda), [], cuda, lr=1e-3, **kw)
        for _ in range(2):
            tr.train_step(inp[0], inp[1], t=inp[2], noise=inp[3])
        torch.cuda.synchronize()
        assert tr.last_grad_norm is None
        sds.append({k: v.detach().clone() for k, v in tr.model.state_dict().items()})
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k
    assert "ldm_adam_step" in called and "ldm_unscale_check" in called
    new = {"ldm_unscale_check_norm", "ldm_grad_norm_finalize", "ldm_adam_step_ext", "ldm_adam_step_dev_ext",
           "ldm_ema_update"}
    assert not (called & new), called & new


# ---- 5. scaler interplay --------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True])
def test_scaler_skips_on_inf_then_clips_a_clean_step(cuda, capturable):
    from ldm_amd import optim as hoptim
    ps = _params(cuda)
    start = [p.detach().clone() for p in ps]
    opt = hoptim.AdamW(ps, lr=5e-3, capturable=capturable)
    opt.attach_ema(DECAY)
    sc = hoptim.GradScaler("cuda", init_scale=1024.0)
    bad = R.grads(400)
    bad[5][777] = np.inf
    _set_grads(ps, bad, cuda, 1024.0)
    sc.unscale_(opt, max_norm=MAX_NORM)
    sc.step(opt)
    sc.update()
    torch.cuda.synchronize()
    assert int(sc._found_inf.item()) == 1 and sc.get_scale() == 512.0
    for p, s in zip(ps, start):
        st = opt.state[p]
        assert torch.equal(p.detach(), s) and torch.equal(st["ema"], s)
        assert float(st.get("step", 0.0)) == 0.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert k not in st or not bool(st[k].any())
    # a clean step at the backed-off scale: clipped and applied
    gs = R.grads(401)
    _set_grads(ps, gs, cuda, 512.0)
    sc.unscale_(opt, max_norm=MAX_NORM)
    sc.step(opt)
    sc.update()
    torch.cuda.synchronize()
    assert int(sc._found_inf.item()) == 0
    norm = R.grad_norm(gs)
    coef = R.clip_coef(norm, MAX_NORM)
    assert coef < 1.0
    assert R.ulp_distance(np.float32(sc.last_grad_norm.item()), np.float32(norm)) <= 1
    for p, s, g in zip(ps, start, gs):
        want, _, _ = R.adam_step(s.cpu().numpy(), g, 0.0 * g, 0.0 * g, 1, 5e-3, weight_decay=1e-2, decoupled=True,
                                 coef=coef)
        assert rel_err(p.detach().double().cpu().numpy(), want) < 1e-6
        assert rel_err(opt.state[p]["ema"].double().cpu().numpy(), R.ema_step(s.cpu().numpy(), want, DECAY)) < 1e-6
        assert float(opt.state[p]["step"]) == 1.0
        assert np.array_equal(p.grad.cpu().numpy(), g)     # unscaled in place, not clipped in memory


def test_buffers_are_not_built_while_capturing(cuda):
    from ldm_amd import optim as hoptim
    from ldm_amd.graphs import capture
    gs = [torch.randn(1000, device=cuda), torch.randn(5000, device=cuda)]
    ps = [torch.nn.Parameter(torch.randn_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g
    hoptim.scale_tensors_(gs, 1.0)           # the chunk map of this size list: built eagerly
    opt = hoptim.Adam(ps, lr=1e-3, capturable=True)
    opt.attach_ema(0.9)                      # the pointer array of the full parameter list
    torch.cuda.synchronize()
    hoptim._norm_cache.clear()
    tables = hoptim.reserve_capture_buffers(device=cuda)     # so that the slot tables themselves can be built
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="gradient-norm buffers are allocated outside a graph capture"):
        with capture(g):
            hoptim.clip_grad_norm_(ps, 1.0)
    torch.cuda.synchronize()
    opt.state[ps[1]]["ema"] = opt.state[ps[1]]["ema"].clone()   # another EMA tensor needs another pointer array
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="EMA pointer array is built outside a graph capture"):
        with capture(g):
            opt.step()
    torch.cuda.synchronize()
    hoptim.release_captured(tables)


# ---- 6. trainer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trainer_runs(cuda):
    """An eager and a graphed trainer after five steps each from the same start (the graphed one: two eager
    warm-up steps, then the capture and three replays), clipping and EMA on."""
    import models.train as TR
    inp = _inputs(cuda, 920)
    runs = {}
    for graph in (False, True):
        tr = TR.LDMTrainer(_model(cuda), [], cuda, lr=1e-3, max_grad_norm=1e-2, ema_decay=0.9)
        tr.autocast_enabled = False
        tr.graph_step = graph
        norms = []
        for _ in range(5):
            tr.train_step(inp[0], inp[1], t=inp[2], noise=inp[3])
            norms.append(tr.last_grad_norm.clone())
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        runs[graph] = (tr, norms)
    return runs, inp


def test_trainer_graphed_equals_eager_bitwise(trainer_runs):
    runs, _ = trainer_runs
    (te, ne), (tg, ng) = runs[False], runs[True]
    for a, b in zip(ne, ng):
        assert a.dim() == 0 and a.device.type == "cuda"
        assert torch.equal(a, b)
        assert float(a) > 1e-2              # the clip bites at every step
    named_e, named_g = dict(te.model.named_parameters()), dict(tg.model.named_parameters())
    moved = 0.0
    for k, pe in named_e.items():
        pg = named_g[k]
        assert torch.equal(pe.detach(), pg.detach()), k
        if pe.requires_grad:
            ee, eg = te.optimizer.state[pe]["ema"], tg.optimizer.state[pg]["ema"]
            assert torch.equal(ee, eg), k
            moved = max(moved, float((ee - pe.detach()).abs().max()))
    assert moved > 0.0


def test_ema_weights_swap_and_state_dict(cuda, trainer_runs):
    import models.train as TR
    runs, inp = trainer_runs
    tr = runs[True][0]
    m = tr.model

    def forward():
        m.eval()
        with torch.no_grad():
            out = m(inp[0], inp[1], inp[2], noise=inp[3])["reconstructed"].clone()
        m.train()
        return out

    raw = {k: v.detach().clone() for k, v in m.state_dict().items()}
    outside = forward()
    with tr.ema_weights():
        inside = forward()
        esd = tr.ema_state_dict()
        for k, p in m.named_parameters():
            if p.requires_grad:
                assert torch.equal(p.detach(), tr.optimizer.state[p]["ema"]), k
    assert not torch.equal(inside, outside)
    for k, v in m.state_dict().items():
        assert torch.equal(v, raw[k]), k
    assert torch.equal(forward(), outside)            # the caches re-packed the raw weights
    assert set(esd) == set(raw)
    # state-dict round trip: the EMA travels; without the key it is re-initialised from the parameters
    sd = copy.deepcopy(tr.optimizer.state_dict())
    assert all("ema" in st for st in sd["state"].values())
    other = TR.LDMTrainer(_model(cuda), [], cuda, lr=1e-3, max_grad_norm=1e-2, ema_decay=0.9)
    other.optimizer.load_state_dict(copy.deepcopy(sd))
    for a, b in zip(tr._trainable, other._trainable):
        assert torch.equal(tr.optimizer.state[a]["ema"], other.optimizer.state[b]["ema"])
    for st in sd["state"].values():
        del st["ema"]
    other.optimizer.load_state_dict(sd)
    for b in other._trainable:
        assert torch.equal(other.optimizer.state[b]["ema"], b.detach())
