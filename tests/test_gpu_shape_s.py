"""SURVEY.md §0.4 / §8(d) secondary stress shape S at its full size: UNet(1, 1) on the raw [B,1,128,512] mel with
style maps s5 [B,256,32,128], s6 [B,512,16,64] (reference model.py:164 default in_channels=1; the cross-attentions
of model.py:140-153 then attend over 4096 (CA2) and 1024 (CA1) tokens, on the KV-tiled flash kernels).

The full size is pinned to the reference itself: tests/golden/ref_goldens_shapeS.npz holds the reference's own
forward on these weights and inputs (make_goldens.py --shapeS; the oracle restatement is pinned to it on the CPU
by tests/test_oracle_golden.py::test_shape_s_full_size_unet).  Checks, all at full size:
* the whole forward (UNet.forward -> _layerwise, what bench.py --workload stress times) against that golden and
  against the oracle in float64 (1e-4, the project's parity bound), and the hipGraph replay of it against the
  golden as well;
* every kernel instance that forward launches -- each conv / transposed conv / 1x1 projection with its epilogue
  on the plan the forward resolved it to, and both attention cores -- replayed alone on fresh inputs against
  float64 (1e-5): test_shape_s_every_layer_instance, which also asserts that the forward still reaches the
  instances it is meant to pin (the Cin = 1 and Cout = 1 convs at 128x512, the flash kernels, the shipped plans);
* the forward's shape, finiteness and bitwise run-to-run determinism, and the graph replay bitwise equal to the
  eager call;
* per-sample independence: a batch of 2 equals its two samples run alone (1e-5; a batch may pick other plans);
* the CA2 attention core at L = S = 4096, E = 256, 4 heads against float64 on a sample of query rows that holds the
  edges of the query tiles and the last row (1e-5);
* one DDIM iteration (the loop body bench.py times) against the DDIM update restated in float64 (1e-6).
Tolerance: fp32 kernels, max |y - y_ref| <= tol * max |y_ref|."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipe
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4          # whole-forward parity bound (test_gpu_parity.py, test_gpu_attention_wide.py)
LAYER_TOL = 1e-5    # one kernel against float64 (test_gpu_bench_config.py)

# query rows every 4096-token sample holds: first / last row, both sides of the 64- and 128-row tile edges and of
# the middle of the sequence, the first row of the last 64-row tile
EDGE_ROWS = (0, 63, 64, 127, 2047, 2048, 4032, 4095)


def _unet(cuda):
    import models.model as M
    u = M.UNet(1, 1, 64)
    recipe.fill_module(u, seed=105)
    return u.to(cuda).eval()


def _inputs(B, cuda, seed=0):
    z = torch.from_numpy(recipe.normal((B, 1, 128, 512), 780 + seed)).to(cuda)
    s5 = torch.from_numpy(recipe.uniform01((B, 256, 32, 128), 781 + seed)).to(cuda)
    s6 = torch.from_numpy(recipe.uniform01((B, 512, 16, 64), 782 + seed)).to(cuda)
    return z, s5, s6


def _cpu_threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


@functools.lru_cache(maxsize=None)
def _golden_out():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_goldens_shapeS.npz"))
    assert g["shapeS_full_t"].tolist() == [117]
    return g["shapeS_full_out"]


@functools.lru_cache(maxsize=None)
def _oracle64_out():
    """The oracle's UNet in float64 on the CPU, on the recipe weights and inputs of _unet / _inputs(1, .)."""
    import models.model as M
    from oracle import ldm_torch_cpu as TC
    _cpu_threads()
    shapes = {k: tuple(v.shape) for k, v in M.UNet(1, 1, 64).state_dict().items()}
    sd = {k: torch.from_numpy(v).double() for k, v in recipe.make_state(shapes, 105).items()}
    z = torch.from_numpy(recipe.normal((1, 1, 128, 512), 780)).double()
    s5 = torch.from_numpy(recipe.uniform01((1, 256, 32, 128), 781)).double()
    s6 = torch.from_numpy(recipe.uniform01((1, 512, 16, 64), 782)).double()
    with torch.no_grad():
        return TC.unet(sd, z, torch.tensor([117]), s5, s6, p="").numpy()


def test_unet_shape_s_full_size_forward_and_graph(cuda):
    from ldm_amd.graphs import capture
    u = _unet(cuda)
    z, s5, s6 = _inputs(1, cuda)
    t = torch.tensor([117], device=cuda)
    emb = {"s5": s5, "s6": s6}
    with torch.no_grad():
        y1 = u(z, t, emb)
        y2 = u(z, t, emb)
        torch.cuda.synchronize()
        assert tuple(y1.shape) == (1, 1, 128, 512)
        assert bool(torch.isfinite(y1).all()) and float(y1.abs().max()) > 0
        assert torch.equal(y1, y2)
        g = torch.cuda.CUDAGraph()
        with capture(g):
            yg = u(z, t, emb)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(yg, y1)
    e_graph = rel_err(yg.cpu().numpy(), _golden_out())
    print(f"\nshape S graph replay vs reference golden: {e_graph:.2e}")
    assert e_graph < TOL


def test_unet_shape_s_full_size_matches_reference(cuda):
    """The forward bench.py --workload stress times (UNet.forward -> _layerwise: the engine does not take a latent
    width of 1) against the reference's own output and against the oracle in float64."""
    from ldm_amd.engine import UNetEngine
    assert not UNetEngine.supports(1)
    u = _unet(cuda)
    z, s5, s6 = _inputs(1, cuda)
    t = torch.tensor([117], device=cuda)
    with torch.no_grad():
        y = u(z, t, {"s5": s5, "s6": s6})
        torch.cuda.synchronize()
    y = y.cpu().numpy()
    gold, o64 = _golden_out(), _oracle64_out()
    e_gold, e_o64, e_ref = rel_err(y, gold), rel_err(y, o64), rel_err(gold, o64)
    print(f"\nshape S full size: ours vs reference golden {e_gold:.2e}, ours vs oracle float64 {e_o64:.2e}, "
          f"reference golden vs oracle float64 (the reference's own fp32 error) {e_ref:.2e}")
    assert e_gold < TOL
    assert e_o64 < TOL


def test_unet_shape_s_per_sample_independence(cuda):
    u = _unet(cuda)
    za, s5a, s6a = _inputs(1, cuda, 0)
    zb, s5b, s6b = _inputs(1, cuda, 10)
    t = torch.tensor([150, 20], device=cuda)
    with torch.no_grad():
        y2 = u(torch.cat([za, zb]), t, {"s5": torch.cat([s5a, s5b]), "s6": torch.cat([s6a, s6b])})
        ya = u(za, t[:1], {"s5": s5a, "s6": s6a})
        yb = u(zb, t[1:], {"s5": s5b, "s6": s6b})
        torch.cuda.synchronize()
    assert rel_err(y2[0:1].cpu().numpy(), ya.cpu().numpy()) < 1e-5
    assert rel_err(y2[1:2].cpu().numpy(), yb.cpu().numpy()) < 1e-5


def _sample_rows(L, seed):
    """Deterministic query rows: every row up to 1024 tokens, else EDGE_ROWS plus 192 random ones."""
    if L <= 1024:
        return np.arange(L)
    rnd = np.random.Generator(np.random.PCG64(seed)).choice(L, 192, replace=False)
    return np.unique(np.concatenate([np.asarray([r for r in EDGE_ROWS if r < L]), rnd]))


def _attention_rows_f64(q, kv, heads, rows):
    """float64 softmax((q sqrt(1/d))^T k) v per head for the query rows `rows` of q [1,E,L], kv [1,2E,S] (the
    layout ops.attention_core takes), on the tensors' device -> [E, len(rows)]."""
    E = q.shape[1]
    d = E // heads
    qd = q.double()[0][:, rows]                                 # [E, R]
    k = kv.double()[0, :E]                                      # [E, S]
    v = kv.double()[0, E:]
    ref = torch.empty(E, rows.numel(), dtype=torch.float64, device=q.device)
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        s = (qd[sl] * math.sqrt(1.0 / d)).t() @ k[sl]           # [R, S]
        p = torch.softmax(s, dim=-1)
        ref[sl] = (p @ v[sl].t()).t()
    return ref


def test_ca2_attention_core_4096_tokens_vs_float64(cuda):
    from ldm_amd import ops
    E, heads, L = 256, 4, 4096
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(1, E, L, generator=g) * 0.5).to(cuda)
    kv = (torch.randn(1, 2 * E, L, generator=g) * 0.5).to(cuda)
    assert ops.attention_uses_flash(E, heads, L, L)
    out = ops.attention_core(q, kv, heads)
    torch.cuda.synchronize()
    rows = _sample_rows(L, 6)
    assert set(EDGE_ROWS) <= set(rows.tolist()) and len(rows) >= 192
    rows = torch.from_numpy(rows).to(cuda)
    ref = _attention_rows_f64(q, kv, heads, rows)
    got = out[0][:, rows].double()
    assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) < 1e-5


def test_shape_s_ddim_iteration_vs_float64_update(cuda):
    """The loop body bench.py --workload stress replays: eps = UNet(1, 1)(x, t), then the reference's DDIM update
    (model.py:442-458) — checked against the update restated in float64 on the same eps."""
    import models.model as M
    from ldm_amd import ops
    u = _unet(cuda)
    z, s5, s6 = _inputs(1, cuda, 20)
    sched = M.ForwardDiffusion()
    times = torch.linspace(sched.num_timesteps - 1, 0, 50).long()
    coefs = sched.reverse_coefs(times).to(cuda)
    t = times[:1].to(cuda)
    x = z.clone()
    x0 = torch.empty_like(x)
    el = torch.empty_like(x)
    with torch.no_grad():
        eps = u(x, t, {"s5": s5, "s6": s6})
        ops.ddim_step_(x, eps, coefs[0].contiguous(), 0.0, x0, el)
        torch.cuda.synchronize()
    ab = sched.alpha_bar_t.double().cpu() if hasattr(sched, "alpha_bar_t") else None
    if ab is None:
        pytest.skip("schedule attribute not found")
    a_t, a_n = ab[int(times[0])], ab[int(times[1])]
    e64 = eps.double().cpu()
    x064 = (z.double().cpu() - (1 - a_t).sqrt() * e64) / a_t.sqrt()
    xn64 = a_n.sqrt() * x064 + (1 - a_n).sqrt() * e64
    assert torch.equal(el, eps)
    assert rel_err(x0.cpu().numpy(), x064.numpy()) < 1e-6
    assert rel_err(x.cpu().numpy(), xn64.numpy()) < 1e-6


# ---- every kernel instance of the full-size forward, alone, against float64 ------------------------------------
# (Cin, Hin, Win, Cout, k, stride, pad, out_pad, transposed) of the UNet's nine convs at B = 1 on a 128x512 mel
# (reference model.py:170-190) and of the cross-attentions' 1x1 projections over 4096 (CA2) / 1024 (CA1) pixels
CONV_LAYERS = {
    "enc1": (1, 128, 512, 64, 3, 1, 1, 0, 0), "enc2": (64, 128, 512, 128, 3, 2, 1, 0, 0),
    "enc3": (128, 64, 256, 256, 3, 2, 1, 0, 0), "enc4": (256, 32, 128, 512, 3, 2, 1, 0, 0),
    "bottleneck": (512, 16, 64, 512, 3, 1, 1, 0, 0), "dec4": (512, 16, 64, 256, 3, 2, 1, 1, 1),
    "dec3": (256, 32, 128, 128, 3, 2, 1, 1, 1), "dec2": (128, 64, 256, 64, 3, 2, 1, 1, 1),
    "dec1": (64, 128, 512, 1, 3, 1, 1, 0, 0)}
PROJ_LAYERS = {
    "ca2.q/out": (256, 32, 128, 256, 1, 1, 0, 0, 0), "ca2.kv": (256, 32, 128, 512, 1, 1, 0, 0, 0),
    "ca1.q/out": (512, 16, 64, 512, 1, 1, 0, 0, 0), "ca1.kv": (512, 16, 64, 1024, 1, 1, 0, 0, 0)}
GROUPS = {"encoder": ("enc1", "enc2", "enc3", "enc4"), "decoder": ("dec4", "dec3", "dec2", "dec1"),
          "attention": ()}   # "middle": the bottleneck, the projections and anything the tables above do not name


class _Recorder:
    """Records, in call order, the ops.conv_forward calls and the attention-core calls of one forward:
    convs as dicts (B, geometry, act, which epilogue operands are present, operand dtype, the plan the call
    resolved to), attention calls as (entry point, B, E, heads, L, S)."""

    ATTN = ("attention_core", "attention_forward_lse")

    def __init__(self, ops):
        self.ops = ops
        self.convs, self.attn = [], []
        self._orig = {n: getattr(ops, n) for n in ("conv_forward",) + self.ATTN}

    def __enter__(self):
        ops, fwd = self.ops, self._orig["conv_forward"]

        def conv_forward(x, weight, bias=None, **kw):
            y = fwd(x, weight, bias, **kw)
            tr = bool(kw.get("transposed", False))
            d = ops.make_desc(x.shape[0], x.shape[1], x.shape[2], x.shape[3], y.shape[1], weight.shape[2],
                              weight.shape[3], kw.get("stride", 1), kw.get("padding", 1),
                              kw.get("output_padding", 0), tr)
            dt = ops.autocast_dt() if kw.get("dtype") is None else int(kw["dtype"])
            adds = kw.get("bcast") is not None or kw.get("skip") is not None
            plan = kw.get("plan") or ops.tiled_plan(d, dt, adds=adds) or ops.get_plan(d)   # as ops.conv_forward
            self.convs.append(dict(
                B=d.B, geom=(d.Cin, d.Hin, d.Win, d.Cout, d.kh, d.stride, d.pad, d.out_pad, d.transposed),
                square=d.kh == d.kw, act=kw.get("act", "none"), bias=bias is not None, bn=kw.get("bn") is not None,
                bcast=kw.get("bcast") is not None, skip=kw.get("skip") is not None, dt=dt,
                forced_plan=kw.get("plan") is not None, desc_key=tuple(d.key()), plan_key=tuple(plan.key())))
            return y

        def attn(name):
            orig = self._orig[name]

            def call(q, kv, heads):
                self.attn.append((name, q.shape[0], q.shape[1], int(heads), q.shape[2], kv.shape[2]))
                return orig(q, kv, heads)
            return call

        ops.conv_forward = conv_forward
        for n in self.ATTN:
            setattr(ops, n, attn(n))
        return self

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(self.ops, n, f)
        return False


_RECORDED = {}


def _recorded(cuda):
    """The calls of ONE full-size forward (recorded once per session, shared by the layer groups)."""
    if "rec" not in _RECORDED:
        from ldm_amd import ops
        u = _unet(cuda)
        z, s5, s6 = _inputs(1, cuda)
        with torch.no_grad(), _Recorder(ops) as rec:
            u(z, torch.tensor([117], device=cuda), {"s5": s5, "s6": s6})
        torch.cuda.synchronize()
        _RECORDED["rec"] = rec
    return _RECORDED["rec"]


def _layer_name(c):
    for table in (CONV_LAYERS, PROJ_LAYERS):
        for name, geom in table.items():
            if c["B"] == 1 and c["geom"] == geom:
                return name
    return "conv" + str(c["geom"])


def _distinct(calls):
    seen, out = set(), []
    for c in calls:
        k = tuple(sorted(c.items())) if isinstance(c, dict) else c
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def _check_coverage(rec):
    """Fails when the forward stops reaching what this test is meant to pin."""
    from ldm_amd import autotune, ops
    convs = rec.convs
    assert all(c["dt"] == 0 and not c["bn"] and not c["forced_plan"] and c["square"] for c in convs), convs
    geoms = [c["geom"] for c in convs if c["B"] == 1]
    # the UNet's nine convs (enc1-4, bottleneck, dec4-1), each at its full-size descriptor, and the six 1x1
    # projections of the two cross-attentions (q and out share a descriptor: four distinct ones)
    for name, geom in {**CONV_LAYERS, **PROJ_LAYERS}.items():
        assert geom in geoms, (name, geoms)
    assert sum(g[4] == 3 for g in geoms) >= 9 and sum(g[4] == 1 for g in geoms) >= 6, geoms
    assert len(convs) >= 15
    # the Cin = 1 stride-1 conv and the Cout = 1 k3 conv at 128x512
    assert any(g[0] == 1 and g[1:3] == (128, 512) and g[4:6] == (3, 1) and not g[8] for g in geoms)
    assert any(g[3] == 1 and g[1:3] == (128, 512) and g[4] == 3 and not g[8] for g in geoms)
    # epilogues as the reference's forward has them: relu(enc2) + t_emb, relu(dec) + skip, dec1 plain
    by = {_layer_name(c): c for c in convs}
    assert by["enc2"]["bcast"] and by["enc2"]["act"] == "relu"
    assert all(by[n]["skip"] and by[n]["act"] == "relu" for n in ("dec4", "dec3", "dec2"))
    assert by["dec1"]["act"] == "none" and by["enc1"]["act"] == "relu" and all(c["bias"] for c in convs)
    # both cross-attentions on the KV-tiled flash kernels
    shapes = sorted({a[1:] for a in rec.attn})
    assert shapes == [(1, 256, 4, 4096, 4096), (1, 512, 4, 1024, 1024)], rec.attn
    for _, E, heads, L, S in shapes:
        assert ops.attention_uses_flash(E, heads, L, S), (E, heads, L, S)
    # the shipped plan-override table: where it has an entry for a recorded descriptor, the forward ran that plan
    with open(autotune.TUNED_PATH) as f:
        table = {tuple(int(s) for s in k.split(",")): tuple(v) + (1,) * (5 - len(v))
                 for k, v in json.load(f).get("plans", {}).items()}
    hits = [c for c in convs if c["desc_key"] in table]
    for c in hits:
        assert c["plan_key"] == table[c["desc_key"]], (_layer_name(c), c["plan_key"], table[c["desc_key"]])
    return len({c["desc_key"] for c in hits})


def _replay_conv(ops, c, seed, cuda):
    """One recorded conv call alone on fresh recipe inputs through ops.conv_forward with the same epilogue
    arguments -> (rel. error against float64 F.conv2d / F.conv_transpose2d + the epilogue, plan key)."""
    Cin, Hin, Win, Cout, k, stride, pad, op, tr = c["geom"]
    B = c["B"]
    bound = math.sqrt(3.0 / (Cin * k * k))                     # unit-variance outputs for unit-variance inputs
    w = torch.from_numpy((recipe.uniform01((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), seed) * 2 - 1) * bound)
    x = torch.from_numpy(recipe.normal((B, Cin, Hin, Win), seed + 1))
    d = ops.make_desc(B, Cin, Hin, Win, Cout, k, k, stride, pad, op, tr)
    yshape = (B, Cout, d.Hout, d.Wout)
    bias = torch.from_numpy(recipe.normal((Cout,), seed + 2) * np.float32(0.5)) if c["bias"] else None
    bcast = torch.from_numpy(recipe.normal((B, Cout), seed + 3)) if c["bcast"] else None
    skip = torch.from_numpy(recipe.normal(yshape, seed + 4)) if c["skip"] else None
    plan_key = tuple(ops.get_plan(d).key())
    assert plan_key == c["plan_key"], (plan_key, c["plan_key"])

    def dev(t):
        return None if t is None else t.to(cuda)
    y = ops.conv_forward(dev(x), dev(w), dev(bias), stride=stride, padding=pad, transposed=bool(tr), output_padding=op,
                         act=c["act"], bcast=dev(bcast), skip=dev(skip), dtype=0)
    torch.cuda.synchronize()
    assert tuple(y.shape) == yshape
    b64 = None if bias is None else bias.double()
    if tr:
        ref = F.conv_transpose2d(x.double(), w.double(), b64, stride=stride, padding=pad, output_padding=op)
    else:
        ref = F.conv2d(x.double(), w.double(), b64, stride=stride, padding=pad)
    assert c["act"] in ("none", "relu")
    if c["act"] == "relu":
        ref = ref.clamp_min(0)
    if bcast is not None:
        ref = ref + bcast.double()[:, :, None, None]
    if skip is not None:
        ref = ref + skip.double()
    return rel_err(y.cpu().numpy(), ref.numpy()), plan_key


def _replay_attention(ops, call, seed, cuda):
    """One recorded attention-core call alone, through the entry point the forward used, against float64 softmax
    attention on the CPU in the call's own layout (q [B,E,L], kv [B,2E,S])."""
    name, B, E, heads, L, S = call
    q = torch.from_numpy(recipe.normal((B, E, L), seed) * np.float32(0.5))
    kv = torch.from_numpy(recipe.normal((B, 2 * E, S), seed + 1) * np.float32(0.5))
    out = getattr(ops, name)(q.to(cuda), kv.to(cuda), heads)
    out = out[0] if isinstance(out, tuple) else out
    torch.cuda.synchronize()
    rows = _sample_rows(L, seed + 2)
    if L > 1024:
        assert set(r for r in EDGE_ROWS if r < L) <= set(rows.tolist()) and len(rows) >= 192
    rows = torch.from_numpy(rows)
    err = 0.0
    for b in sorted({0, B - 1}):
        ref = _attention_rows_f64(q[b:b + 1], kv[b:b + 1], heads, rows)
        err = max(err, rel_err(out[b][:, rows.to(cuda)].cpu().numpy(), ref.numpy()))
    return err, len(rows)


@pytest.mark.parametrize("group", ["encoder", "middle", "decoder", "attention"])
def test_shape_s_every_layer_instance(cuda, group):
    """Every distinct ops.conv_forward call and attention-core call of one full-size B = 1 forward, replayed alone
    on fresh recipe inputs on the plan the forward resolved it to, against float64 (1e-5), one layer group per
    case; every case first asserts the coverage of the recording (_check_coverage)."""
    from ldm_amd import ops
    rec = _recorded(cuda)
    n_table = _check_coverage(rec)
    _cpu_threads()
    rows, bad = [], []
    if group == "attention":
        for i, call in enumerate(_distinct(rec.attn)):
            err, n = _replay_attention(ops, call, 9100 + 10 * i, cuda)
            rows.append(f"{call[0]} B={call[1]} E={call[2]} heads={call[3]} L={call[4]} S={call[5]} "
                        f"({n} query rows): {err:.2e}")
            if not err < LAYER_TOL:
                bad.append(rows[-1])
    else:
        named = [n for g in GROUPS.values() for n in g]
        for i, c in enumerate(_distinct(rec.convs)):
            name = _layer_name(c)
            if (name in GROUPS[group]) if group != "middle" else (name not in named):
                err, plan_key = _replay_conv(ops, c, 9000 + 10 * i, cuda)
                epi = c["act"] + ("+bcast" if c["bcast"] else "") + ("+skip" if c["skip"] else "")
                rows.append(f"{name} {c['geom']} {epi} plan {plan_key}: {err:.2e}")
                if not err < LAYER_TOL:
                    bad.append(rows[-1])
    print(f"\nshape S {group} instances ({n_table} recorded descriptors in the shipped plan table):\n" +
          "\n".join(rows))
    assert rows, group
    assert not bad, bad
