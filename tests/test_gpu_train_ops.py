"""GPU: the train path's scalar kernels (csrc/misc.hip: loss forward / backward, q_sample, predict_start, their
backward, eval BatchNorm, activations, the sinusoid and the time MLP's t switch) and the frozen-BatchNorm branch of
functional._conv_backward, each called directly and held elementwise to the float64 yardstick tests/train_ops_ref.py.

The bars are derived, not measured: U = 2^-24, and a bar of k U on elem_err allows k/2 fp32 roundings of operands of
the stated per-element magnitude (see the yardstick's header); the transcendental functions get the absolute 1e-6
of their documented few-ulp error.  The inputs come from the yardstick module and are checked on the CPU in
tests/test_train_ops_host.py.
"""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    """The tensor's float32 bit patterns on the host (NaN-safe, sign-of-zero-exact equality)."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def table(cuda):
    return T(R.coef_table(), cuda)


# ---- losses ----------------------------------------------------------------------------------------------
def _loss_ref(kind, a, b):
    if kind == 0:
        ref = R.mse(a, b)
        return ref, R.loss_bar(ref, R.mse_term_mag(a, b))
    ref = R.kl(a)
    return ref, R.loss_bar(ref, R.kl_term_mag(a))


@pytest.mark.parametrize("n", R.LOSS_N)
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_forward(cuda, kind, n):
    """n = 1 thread, a partial wave, one block (exact, +1), exactly 512 full blocks, one element into the second
    grid-stride pass, more than two passes; twice bitwise equal."""
    from ldm_amd import ops
    a, b = R.loss_inputs(kind, n)
    ag, bg = T(a, cuda), (None if b is None else T(b, cuda))
    y1 = ops.loss_forward(kind, ag, bg)
    y2 = ops.loss_forward(kind, ag, bg)
    assert y1.shape == () and y1.dtype == torch.float32 and same_bits(y1, y2)
    ref, bar = _loss_ref(kind, a, b)
    err = abs(float(y1.double().item()) - ref)
    print(f"loss kind {kind} n {n}: |err| {err:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("n", R.LOSS_N)
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_backward(cuda, kind, n):
    """Upstream g in {1, 0.37, 65536 (the grad scaler's scale)}; MSE with need_a / need_b in all four combinations
    (an output not asked for is None, the other unchanged bitwise), gb = -ga bitwise; twice bitwise equal."""
    from ldm_amd import ops
    a, b = R.loss_inputs(kind, n)
    ag, bg = T(a, cuda), (None if b is None else T(b, cuda))
    for g in R.LOSS_G:
        gg = torch.tensor(g, device=cuda, dtype=torch.float32)
        if kind == 1:
            ga, gb = ops.loss_backward(1, ag, None, gg, True, False)
            ga2, _ = ops.loss_backward(1, ag, None, gg, True, False)
            assert gb is None and same_bits(ga, ga2)
            err = R.elem_err(npy(ga), R.kl_grad(a, g), R.kl_grad_scale(a, g))
            print(f"kl grad n {n} g {g}: {err / U:.2f} U")
            assert err <= 8 * U
            continue
        ref_a, ref_b = R.mse_grad(a, b, g)
        ga, gb = ops.loss_backward(0, ag, bg, gg, True, True)
        ga2, gb2 = ops.loss_backward(0, ag, bg, gg, True, True)
        assert same_bits(ga, ga2) and same_bits(gb, gb2)
        assert same_bits(gb, -ga)
        ea = R.elem_err(npy(ga), ref_a, np.abs(ref_a))
        eb = R.elem_err(npy(gb), ref_b, np.abs(ref_b))
        print(f"mse grad n {n} g {g}: ga {ea / U:.2f} U, gb {eb / U:.2f} U")
        assert ea <= 8 * U and eb <= 8 * U
        only_a = ops.loss_backward(0, ag, bg, gg, True, False)
        only_b = ops.loss_backward(0, ag, bg, gg, False, True)
        assert only_a[1] is None and same_bits(only_a[0], ga)
        assert only_b[0] is None and same_bits(only_b[1], gb)
        assert ops.loss_backward(0, ag, bg, gg, False, False) == (None, None)


def test_loss_kinds_back_to_back_share_the_workspace(cuda):
    """MSE then KL then MSE on one stream: the three go through one fp64 workspace in stream order, each correct and
    each bitwise what it gives alone."""
    from ldm_amd import ops
    n = 300001
    (a, b), (z, _) = R.loss_inputs(0, n), R.loss_inputs(1, n)
    ag, bg, zg = T(a, cuda), T(b, cuda), T(z, cuda)
    alone_m, alone_k = ops.loss_forward(0, ag, bg), ops.loss_forward(1, zg)
    torch.cuda.synchronize()
    m1, k1, m2 = ops.loss_forward(0, ag, bg), ops.loss_forward(1, zg), ops.loss_forward(0, ag, bg)
    for y, (ref, bar) in ((m1, _loss_ref(0, a, b)), (k1, _loss_ref(1, z, None))):
        assert abs(float(y.double().item()) - ref) <= bar
    assert same_bits(m1, alone_m) and same_bits(m2, alone_m) and same_bits(k1, alone_k)


def test_loss_on_two_streams_has_a_workspace_per_stream(cuda):
    """The pair issued on two streams at once (each waits on an event of the inputs, the reader on an event of each)
    gives the single-stream values bitwise: ops._LOSS_WS keeps one workspace per stream."""
    from ldm_amd import ops
    n = 300001
    (a, b), (z, _) = R.loss_inputs(0, n), R.loss_inputs(1, n)
    ag, bg, zg = T(a, cuda), T(b, cuda), T(z, cuda)
    want_m, want_k = ops.loss_forward(0, ag, bg), ops.loss_forward(1, zg)
    cur = torch.cuda.current_stream(cuda)
    ready = torch.cuda.Event()
    ready.record(cur)
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    outs, done, ws = [[], []], [], []
    for rep in range(8):      # interleaved issue: the two streams' kernels are in flight together
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                if rep == 0:
                    s.wait_event(ready)
                outs[i].append(ops.loss_forward(0, ag, bg) if i == 0 else ops.loss_forward(1, zg))
                if rep == 0:
                    ws.append(ops._LOSS_WS[(str(ag.device), s.cuda_stream)])
    for s in streams:
        ev = torch.cuda.Event()
        ev.record(s)
        done.append(ev)
    for ev in done:
        cur.wait_event(ev)
    assert ws[0].data_ptr() != ws[1].data_ptr()
    assert ws[0].data_ptr() != ops._LOSS_WS[(str(ag.device), cur.cuda_stream)].data_ptr()
    for y in outs[0]:
        assert same_bits(y, want_m)
    for y in outs[1]:
        assert same_bits(y, want_k)
    torch.cuda.synchronize()
    for s in streams:
        ops._LOSS_WS.pop((str(ag.device), s.cuda_stream), None)


@pytest.mark.parametrize("n", [257, 131073])
def test_loss_autograd_delivers_both_gradients(cuda, n):
    """functional.mse_loss with the target requiring grad: .backward() delivers gb (the train step never asks for it);
    functional.kl_loss likewise, with the scaler's upstream gradient."""
    from ldm_amd import functional as HF
    a, b = R.loss_inputs(0, n)
    for g in (1.0, 65536.0):
        ag, bg = T(a, cuda).requires_grad_(), T(b, cuda).requires_grad_()
        loss = HF.mse_loss(ag, bg)
        loss.backward(torch.tensor(g, device=cuda))
        ref_a, ref_b = R.mse_grad(a, b, g)
        assert R.elem_err(npy(ag.grad), ref_a, np.abs(ref_a)) <= 8 * U
        assert R.elem_err(npy(bg.grad), ref_b, np.abs(ref_b)) <= 8 * U
        assert same_bits(bg.grad, -ag.grad)
        # the target alone
        bg2 = T(b, cuda).requires_grad_()
        HF.mse_loss(T(a, cuda), bg2).backward(torch.tensor(g, device=cuda))
        assert same_bits(bg2.grad, bg.grad)
        z, _ = R.loss_inputs(1, n)
        zg = T(z, cuda).requires_grad_()
        HF.kl_loss(zg).backward(torch.tensor(g, device=cuda))
        assert R.elem_err(npy(zg.grad), R.kl_grad(z, g), R.kl_grad_scale(z, g)) <= 8 * U


# ---- scheduler --------------------------------------------------------------------------------------------
def _t_forms(t, dev):
    return {"int64_device": torch.from_numpy(t).to(dev), "int64_host": torch.from_numpy(t),
            "int32_host": torch.from_numpy(t.astype(np.int32))}


@pytest.mark.parametrize("B,per", R.SCHED_SHAPES)
def test_scheduler_forward(cuda, table, B, per):
    """q_sample and predict_start with a distinct t per sample (0 and T - 1 among them) at shapes whose 256-thread
    blocks straddle samples; t as int64 on the device, int64 and int32 on the host give the same bits."""
    from ldm_amd import ops
    tab = R.coef_table()
    a, b, _g, t = R.sched_inputs(B, per)
    ag, bg = T(a, cuda), T(b, cuda)
    for fn, ref, scale, bar in ((ops.q_sample, R.q_sample, R.q_sample_scale, 2 * U),
                                (ops.predict_start, R.predict_start, R.predict_start_scale, 6 * U)):
        ys = {k: fn(ag, bg, table, tt) for k, tt in _t_forms(t, cuda).items()}
        y = ys["int64_device"]
        assert all(same_bits(y, v) for v in ys.values())
        err = R.elem_err(npy(y), ref(a, b, tab, t), scale(a, b, tab, t))
        print(f"{fn.__name__} ({B}, {per}): {err / U:.2f} U")
        assert err <= bar


@pytest.mark.parametrize("B,per", R.SCHED_SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_sched_backward(cuda, table, kind, B, per):
    """Both outputs, ga alone and gb alone (a null pointer in the kernel): the output not asked for is None and the
    other one keeps its bits."""
    from ldm_amd import ops
    tab = R.coef_table()
    _a, _b, g, t = R.sched_inputs(B, per)
    gg = T(g, cuda)
    ref_a, ref_b = R.sched_backward(kind, g, tab, t)
    for name, tt in _t_forms(t, cuda).items():
        ga, gb = ops.sched_backward(kind, gg, table, tt, True, True)
        ea = R.elem_err(npy(ga), ref_a, np.abs(ref_a))
        eb = R.elem_err(npy(gb), ref_b, np.abs(ref_b))
        print(f"sched_backward kind {kind} ({B}, {per}) {name}: ga {ea / U:.2f} U, gb {eb / U:.2f} U")
        assert ea <= 6 * U and eb <= 6 * U
        only_a = ops.sched_backward(kind, gg, table, tt, True, False)
        only_b = ops.sched_backward(kind, gg, table, tt, False, True)
        assert only_a[1] is None and same_bits(only_a[0], ga)
        assert only_b[0] is None and same_bits(only_b[1], gb)


@pytest.mark.parametrize("B,per", [(5, 257), (4, 255)])
def test_scheduler_autograd(cuda, table, B, per):
    """functional.q_sample / predict_start: autograd to both inputs, and to each alone."""
    from ldm_amd import functional as HF
    tab = R.coef_table()
    a, b, g, t = R.sched_inputs(B, per)
    tg, gg = T(t, cuda), T(g, cuda)
    for kind, fn in ((0, HF.q_sample), (1, HF.predict_start)):
        ref_a, ref_b = R.sched_backward(kind, g, tab, t)
        ag, bg = T(a, cuda).requires_grad_(), T(b, cuda).requires_grad_()
        fn(ag, bg, table, tg).backward(gg)
        assert R.elem_err(npy(ag.grad), ref_a, np.abs(ref_a)) <= 6 * U
        assert R.elem_err(npy(bg.grad), ref_b, np.abs(ref_b)) <= 6 * U
        a1, b1 = T(a, cuda).requires_grad_(), T(b, cuda).requires_grad_()
        fn(a1, T(b, cuda), table, tg).backward(gg)
        fn(T(a, cuda), b1, table, tg).backward(gg)
        assert same_bits(a1.grad, ag.grad) and same_bits(b1.grad, bg.grad)


@pytest.mark.parametrize("per", [7, 257])
def test_scheduler_out_of_range_t_poisons_its_sample_only(cuda, table, per):
    """The documented rule (misc.hip load_coef): t outside [0, T) makes that sample NaN -- forward and backward --
    and the table is not read for it; the other samples keep the in-range run's bits."""
    from ldm_amd import ops
    B = 5
    a, b, g, t = R.sched_inputs(B, per)
    bad = t.copy()
    bad[1], bad[3] = -1, R.SCHED_T
    ag, bg, gg = T(a, cuda), T(b, cuda), T(g, cuda)
    runs = {
        "q_sample": lambda tt: (ops.q_sample(ag, bg, table, tt),),
        "predict_start": lambda tt: (ops.predict_start(ag, bg, table, tt),),
        "backward0": lambda tt: ops.sched_backward(0, gg, table, tt),
        "backward1": lambda tt: ops.sched_backward(1, gg, table, tt),
    }
    for name, run in runs.items():
        good, poisoned = run(T(t, cuda)), run(T(bad, cuda))
        for yg, yp in zip(good, poisoned):
            assert torch.isfinite(yg).all(), name
            assert torch.isnan(yp[[1, 3]]).all(), name
            assert same_bits(yp[[0, 2, 4]], yg[[0, 2, 4]]), name


# ---- eval BatchNorm ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", R.ACT_NAMES)
@pytest.mark.parametrize("B,C,HW", R.BN_SHAPES)
def test_batchnorm_eval(cuda, B, C, HW, act):
    """Weight and bias present and None (None / None is how the frozen-BN conv backward calls it), C no power of two,
    blocks crossing channel and plane boundaries, running variances from 1e-6 to 10."""
    from ldm_amd import ops
    x, w, b, rm, rv = R.bn_inputs(B, C, HW)
    xg, rmg, rvg = T(x, cuda), T(rm, cuda), T(rv, cuda)
    for wa in (w, None):
        for ba in (b, None):
            y = ops.batchnorm_eval(xg, None if wa is None else T(wa, cuda), None if ba is None else T(ba, cuda),
                                   rmg, rvg, R.BN_EPS, act)
            assert y.shape == xg.shape
            ref = R.bn_eval(x, wa, ba, rm, rv, R.BN_EPS, act)
            bar = R.bn_eval_bar(x, wa, ba, rm, rv, R.BN_EPS, act)
            err = R.elem_err(npy(y), ref, bar)
            print(f"batchnorm_eval {(B, C, HW)} {act} w {wa is not None} b {ba is not None}: {err:.3f} of the bar")
            assert err <= 1.0


# ---- activations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ACT_N)
@pytest.mark.parametrize("act", R.ACT_NAMES)
def test_activation(cuda, act, n):
    """+-0, +-1e-8, +-0.5, +-6, +-20 (tanh saturation, the GELU tails) among uniform values; none / relu exact."""
    from ldm_amd import ops
    for x in R.act_inputs(n):
        y = ops.activation(T(x, cuda), act)
        ref = R.act_np(act, x)
        if act in R.ACT_EXACT:
            assert np.array_equal(npy(y), ref)
            continue
        err = R.elem_err(npy(y), ref, R.act_bar(act, ref))
        print(f"activation {act} n {n}: {err:.3f} of the bar")
        assert err <= 1.0


@pytest.mark.parametrize("n", R.ACT_N)
@pytest.mark.parametrize("act", R.ACT_NAMES)
def test_activation_autograd(cuda, act, n):
    """functional.activation(...).backward() against autograd of the yardstick; upstream |g| <= 1, so the bar is the
    forward's (the derivatives are bounded by 1.13 and are formed from the same functions)."""
    from ldm_amd import functional as HF
    for x in R.act_inputs(n):
        g = R.uniform((n,), 310)
        xt = torch.from_numpy(x).double().requires_grad_()
        R.act(act, xt).backward(torch.from_numpy(g).double())
        ref = xt.grad.numpy()
        xg = T(x, cuda).requires_grad_()
        HF.activation(xg, act).backward(T(g, cuda))
        if act in R.ACT_EXACT:
            assert np.array_equal(npy(xg.grad), ref)
            continue
        err = R.elem_err(npy(xg.grad), ref, 1e-6 * np.maximum(1.0, np.abs(ref)))
        print(f"activation backward {act} n {n}: {err:.3f} of the bar")
        assert err <= 1.0


# ---- time embedding ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.EMBED_DIMS)
def test_time_embedding(cuda, dim):
    """sinusoid_embed against the yardstick (absolute 1e-6: outputs bounded by 1), and t as int64 and as float32
    giving the same bits from sinusoid_embed and from time_mlp (recipe weights)."""
    import recipe
    from ldm_amd import ops
    t = np.array(R.EMBED_T, dtype=np.int64)
    ti, tf = T(t, cuda), T(t.astype(np.float32), cuda)
    e_i, e_f = ops.sinusoid_embed(ti, dim, cuda), ops.sinusoid_embed(tf, dim, cuda)
    assert e_i.shape == (len(t), dim) and same_bits(e_i, e_f)
    assert same_bits(e_i, ops.sinusoid_embed(torch.from_numpy(t), dim, cuda))          # host t
    err = float(np.abs(npy(e_i) - R.sinusoid(t, dim)).max())
    print(f"sinusoid dim {dim}: max abs err {err:.3e}")
    assert err <= 1e-6
    w = {k: T(v, cuda) for k, v in recipe.make_state({"1.weight": (dim, dim), "1.bias": (dim,), "3.weight": (dim, dim),
                                                      "3.bias": (dim,)}, seed=900 + dim).items()}
    args = (w["1.weight"], w["1.bias"], w["3.weight"], w["3.bias"])
    m_i, m_f = ops.time_mlp(ti, *args), ops.time_mlp(tf, *args)
    assert m_i.shape == (len(t), dim) and same_bits(m_i, m_f)
    # ... and the MLP is the float64 one on the yardstick's embedding (1e-5: two dim-long fp32 dot products)
    w64 = {k: npy(v) for k, v in w.items()}
    h = torch.from_numpy(R.sinusoid(t, dim) @ w64["1.weight"].T + w64["1.bias"])
    want = R.act("gelu", h).numpy() @ w64["3.weight"].T + w64["3.bias"]
    assert rel_err(npy(m_i), want) < 1e-5


# ---- conv with a frozen eval-mode BatchNorm in its epilogue -----------------------------------------------------
def _conv_bn_gpu(case, inp, act, dev, grads=("x", "w", "b", "skip")):
    from ldm_amd import functional as HF
    s, p, op, tr = case[6:10]
    x, w, b = (T(inp[k], dev).requires_grad_(k in grads) for k in ("x", "w", "b"))
    bc = None if inp["bcast"] is None else T(inp["bcast"], dev)
    sk = None if inp["skip"] is None else T(inp["skip"], dev).requires_grad_("skip" in grads)
    bn = tuple(T(v, dev) for v in inp["bn"]) + (inp["eps"],)
    y = HF.conv(x, w, b, stride=s, padding=p, transposed=tr, output_padding=op, act=act, bcast=bc, skip=sk, bn_eval=bn)
    (y * T(inp["R"], dev)).sum().backward()
    return y, x, w, b, sk


@pytest.mark.parametrize("act", R.CONV_BN_ACTS)
@pytest.mark.parametrize("name", R.CONV_BN_SHAPES)
def test_conv_frozen_bn_backward(cuda, name, act):
    """functional.conv(..., bn_eval=(w, b, rm, rv, eps)) with gradients flowing: y, dx, dw, db and dskip against
    float64 conv -> BN (running statistics) -> act (+bcast, +skip), at test_conv_backward's bar for the same
    kernels.  The BN weight holds a negative and a zero entry, the running variances span 1e-3 .. 4."""
    from test_gpu_train import CONV_CASES, TOL
    case = CONV_CASES[name]
    inp = R.conv_bn_inputs(case, zlib.crc32(name.encode()) % 1000)
    ref = R.conv_bn(case, inp, act)
    y, x, w, b, sk = _conv_bn_gpu(case, inp, act, cuda)
    errs = {"y": rel_err(npy(y), ref["y"]), "dx": rel_err(npy(x.grad), ref["dx"]),
            "dw": rel_err(npy(w.grad), ref["dw"]), "db": rel_err(npy(b.grad), ref["db"])}
    if sk is not None:
        errs["dskip"] = rel_err(npy(sk.grad), ref["dskip"])
    print(f"frozen-BN conv {name} {act}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert (ref["dskip"] is None) == (sk is None)
    for k, v in errs.items():
        assert v < TOL, k


@pytest.mark.parametrize("name", R.CONV_BN_SHAPES)
def test_conv_frozen_bn_gradient_to_the_input_only(cuda, name):
    """A gradient passing through a frozen eval-mode encoder: only x requires grad, the conv's weights are frozen."""
    from test_gpu_train import CONV_CASES, TOL
    case = CONV_CASES[name]
    inp = R.conv_bn_inputs(case, zlib.crc32(name.encode()) % 1000)
    ref = R.conv_bn(case, inp, "relu")
    y, x, w, b, sk = _conv_bn_gpu(case, inp, "relu", cuda, grads=("x",))
    assert w.grad is None and b.grad is None and (sk is None or sk.grad is None)
    assert rel_err(npy(y), ref["y"]) < TOL
    assert rel_err(npy(x.grad), ref["dx"]) < TOL


def test_conv_bn_act_dispatch(cuda, monkeypatch):
    """models.model._conv_bn_act: a BatchNorm in .eval() with frozen affine is folded into the conv (the bn_eval
    branch, gradients correct); with the affine trainable it runs the stand-alone eval BatchNorm, whose backward has
    no kernel and must raise rather than return a gradient."""
    import models.model as M
    from ldm_amd import functional as HF
    from ldm_amd import nn as hnn
    from test_gpu_train import CONV_CASES, TOL
    case = CONV_CASES["unet_enc1_k3s1"]
    B, Cin, H, W, Cout, k, s, p = case[:8]
    inp = R.conv_bn_inputs(case, 77)
    ref = R.conv_bn(case, inp, "relu")
    conv, bn = hnn.Conv2d(Cin, Cout, k, s, p).to(cuda), hnn.BatchNorm2d(Cout, eps=inp["eps"]).to(cuda)
    with torch.no_grad():
        conv.weight.copy_(T(inp["w"], cuda))
        conv.bias.copy_(T(inp["b"], cuda))
        for dst, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), inp["bn"]):
            dst.copy_(T(v, cuda))
    bn.eval()
    seen = []
    real = HF.conv
    monkeypatch.setattr(HF, "conv", lambda *a, **kw: (seen.append(kw.get("bn_eval")), real(*a, **kw))[1])
    for q in bn.parameters():
        q.requires_grad_(False)
    x = T(inp["x"], cuda).requires_grad_()
    y = M._conv_bn_act(conv, bn, "relu", x)
    assert len(seen) == 1 and seen[0] is not None and seen[0][0] is bn.weight and seen[0][3] is bn.running_var
    (y * T(inp["R"], cuda)).sum().backward()
    assert rel_err(npy(y), ref["y"]) < TOL and rel_err(npy(x.grad), ref["dx"]) < TOL
    assert rel_err(npy(conv.weight.grad), ref["dw"]) < TOL and rel_err(npy(conv.bias.grad), ref["db"]) < TOL
    assert bn.weight.grad is None and bn.bias.grad is None
    # trainable affine, still .eval(): the stand-alone eval BatchNorm
    for q in bn.parameters():
        q.requires_grad_(True)
    seen.clear()
    x2 = T(inp["x"], cuda).requires_grad_()
    y2 = M._conv_bn_act(conv, bn, "relu", x2)
    assert len(seen) == 1 and seen[0] is None
    assert rel_err(npy(y2), ref["y"]) < TOL
    with pytest.raises(NotImplementedError):
        (y2 * T(inp["R"], cuda)).sum().backward()
    assert x2.grad is None and bn.weight.grad is None
