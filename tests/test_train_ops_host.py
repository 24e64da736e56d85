"""CPU: the float64 yardstick of the train path's scalar kernels (tests/train_ops_ref.py) against float64 torch --
closed-form gradients against autograd, eval BatchNorm against nn.BatchNorm2d.eval(), activations against
torch.nn.functional -- and the inputs of tests/test_gpu_train_ops.py themselves: finite in the reference wherever a
sample was not deliberately given an out-of-range timestep."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_ref as R      # noqa: E402

SHAPES = [(3, 7), (2, 5, 13)]
TIGHT = 1e-13


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def close(a, b, tol=TIGHT):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_values_and_closed_form_gradients(shape):
    a, b = R.uniform(shape, 1, -2, 2), R.uniform(shape, 2, -2, 2)
    for g in R.LOSS_G:
        at, bt = t64(a).requires_grad_(), t64(b).requires_grad_()
        loss = tF.mse_loss(at, bt)
        assert abs(R.mse(a, b) - loss.item()) <= TIGHT
        (loss * g).backward()
        ga, gb = R.mse_grad(a, b, g)
        assert close(ga, at.grad, 1e-12) and close(gb, bt.grad, 1e-12)
        zt = t64(a).requires_grad_()
        kl = torch.mean(0.5 * (zt.pow(2) - 1 - torch.log(zt.pow(2) + 1e-8)))
        assert abs(R.kl(a) - kl.item()) <= TIGHT
        (kl * g).backward()
        assert close(R.kl_grad(a, g), zt.grad, 1e-12)
        assert np.all(R.kl_grad_scale(a, g) >= np.abs(R.kl_grad(a, g)) * (1 - 1e-12))


def test_kl_gradient_at_the_special_points():
    """The KL specials change the gradient's scale by 1e8 (a = 1e-4 against a = 1): autograd agrees elementwise."""
    a = np.array(R.KL_SPECIALS, dtype=np.float32)
    zt = t64(a).requires_grad_()
    torch.mean(0.5 * (zt.pow(2) - 1 - torch.log(zt.pow(2) + 1e-8))).backward()
    got, want = R.kl_grad(a, 1.0), zt.grad.numpy()
    assert np.all(np.abs(got - want) <= 1e-12 * R.kl_grad_scale(a, 1.0))
    assert got[0] == 0 and got[1] == 0 and abs(got[2]) > 10      # a = 0 -> 0;  a = 1e-5 -> about -990 / n


@pytest.mark.parametrize("shape", SHAPES)
def test_scheduler_against_autograd(shape):
    tab = R.coef_table()
    assert tab.dtype == np.float32 and tab.shape == (R.SCHED_T, 2)
    assert np.all(np.abs(R.f64(tab) ** 2 @ np.ones(2) - 1.0) < 1e-6)          # sa^2 + s1^2 = 1
    B = shape[0]
    t = R.sched_t(B)
    a, b, g = (R.uniform(shape, 10 + i, -2, 2) for i in range(3))
    sa = t64(tab[t, 0]).reshape((B,) + (1,) * (len(shape) - 1))
    s1 = t64(tab[t, 1]).reshape((B,) + (1,) * (len(shape) - 1))
    at, bt = t64(a).requires_grad_(), t64(b).requires_grad_()
    z = sa * at + s1 * bt
    assert close(R.q_sample(a, b, tab, t), z.detach())
    z.backward(t64(g))
    ga, gb = R.sched_backward(0, g, tab, t)
    assert close(ga, at.grad) and close(gb, bt.grad)
    at, bt = t64(a).requires_grad_(), t64(b).requires_grad_()
    x0 = (at - s1 * bt) / sa
    assert close(R.predict_start(a, b, tab, t), x0.detach())
    x0.backward(t64(g))
    ga, gb = R.sched_backward(1, g, tab, t)
    assert close(ga, at.grad) and close(gb, bt.grad)
    # predict_start inverts q_sample
    assert close(R.predict_start(R.q_sample(a, b, tab, t), b, tab, t), a, 1e-12)
    # the scales bound the results they are the scales of
    assert np.all(R.q_sample_scale(a, b, tab, t) >= np.abs(R.q_sample(a, b, tab, t)))
    assert np.all(R.predict_start_scale(a, b, tab, t) >= np.abs(R.predict_start(a, b, tab, t)) * (1 - 1e-12))


def test_scheduler_out_of_range_poisons_only_its_sample():
    tab = R.coef_table()
    a, b, g, t = R.sched_inputs(5, 7)
    bad = t.copy()
    bad[1], bad[3] = -1, R.SCHED_T
    for fn in (lambda tt: R.q_sample(a, b, tab, tt), lambda tt: R.predict_start(a, b, tab, tt),
               lambda tt: R.sched_backward(0, g, tab, tt)[1], lambda tt: R.sched_backward(1, g, tab, tt)[1]):
        good, poisoned = fn(t), fn(bad)
        assert np.isnan(poisoned[[1, 3]]).all() and np.isfinite(good).all()
        assert np.array_equal(poisoned[[0, 2, 4]], good[[0, 2, 4]])


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 5, 1, 13)])
@pytest.mark.parametrize("affine", [(True, True), (True, False), (False, True), (False, False)])
def test_bn_eval_against_torch(shape, affine):
    B, C = shape[:2]
    x, w, b, rm, rv = R.bn_inputs(B, C, shape[2] * shape[3])
    x = x.reshape(shape)
    bn = torch.nn.BatchNorm2d(C, eps=R.BN_EPS).double().eval()
    with torch.no_grad():
        bn.running_mean.copy_(t64(rm))
        bn.running_var.copy_(t64(rv))
        bn.weight.copy_(t64(w) if affine[0] else torch.ones(C).double())
        bn.bias.copy_(t64(b) if affine[1] else torch.zeros(C).double())
        want = bn(t64(x))
    wa, ba = (w if affine[0] else None), (b if affine[1] else None)
    assert close(R.bn_eval(x, wa, ba, rm, rv, R.BN_EPS), want, 1e-12)
    assert close(R.bn_eval(x, wa, ba, rm, rv, R.BN_EPS, "relu"), torch.relu(want), 1e-12)
    assert np.all(R.bn_eval_scale(x, wa, ba, rm, rv, R.BN_EPS) >= np.abs(want.numpy()) * (1 - 1e-12))


@pytest.mark.parametrize("shape", SHAPES)
def test_activations_against_torch_functional(shape):
    import ldm_amd._lib as L
    assert set(R.ACT_NAMES) == set(L.ACT)
    x = np.concatenate([R.uniform(shape, 20, -4, 4).reshape(-1), np.array(R.ACT_SPECIALS, dtype=np.float32)])
    want = {"none": lambda v: v, "relu": tF.relu, "tanh": torch.tanh, "tanh_half": lambda v: (torch.tanh(v) + 1) / 2,
            "gelu": tF.gelu}
    for name in R.ACT_NAMES:
        xt, xr = t64(x).requires_grad_(), t64(x).requires_grad_()
        y, yr = R.act(name, xt), want[name](xr)
        assert close(y.detach(), yr.detach()), name
        g = t64(R.uniform(x.shape, 21))
        y.backward(g)
        yr.backward(g)
        assert close(xt.grad, xr.grad, 1e-12), name
    # max |act'| as the BatchNorm bar uses it, on a fine grid
    v = torch.linspace(-8, 8, 32001, dtype=torch.float64, requires_grad=True)
    for name in R.ACT_NAMES:
        (gr,) = torch.autograd.grad(R.act(name, v).sum(), v)
        assert gr.abs().max().item() <= R.ACT_LIPSCHITZ[name], name


@pytest.mark.parametrize("dim", R.EMBED_DIMS)
def test_sinusoid_against_the_model_formula(dim):
    """The yardstick's argument is the float32 product the model forms (SinusoidalPositionEmbeddings: time[:, None] *
    embeddings[None, :] in float32); with sin / cos in float64 it sits within float32's own sin / cos error of the
    model's float32 embedding, and its table is the one the kernels are handed."""
    from ldm_amd import ops
    f = R.sinusoid_freqs(dim)
    assert f.dtype == np.float32 and np.array_equal(f, ops.sinusoid_freqs(dim, "cpu").numpy())
    half = dim // 2
    exact = np.exp(np.arange(half) * -(np.log(10000.0) / (half - 1)))
    # float32 exponent: the step and the product each rounded once (|arg| <= ln 1e4), then exp's own rounding
    assert np.all(np.abs(f - exact) <= (2 * np.log(10000.0) + 2) * R.U * exact)
    t = torch.tensor(R.EMBED_T)
    arg = t.float()[:, None] * torch.from_numpy(f)[None, :]
    model = torch.cat((arg.sin(), arg.cos()), dim=-1)
    got = R.sinusoid(R.EMBED_T, dim)
    assert got.shape == (len(R.EMBED_T), dim) and np.abs(got - model.double().numpy()).max() <= 2e-7
    assert np.array_equal(got, R.sinusoid(np.array(R.EMBED_T, dtype=np.float32), dim))
    assert np.all(got[0, :half] == 0) and np.all(got[0, half:] == 1)


def test_elem_err():
    ref = np.array([1.0, 1e-6, 0.0])
    assert R.elem_err(ref, ref, np.abs(ref)) == 0.0
    assert R.elem_err(ref + np.array([0, 1e-9, 0]), ref, np.abs(ref)) == pytest.approx(1e-3)   # small element seen
    assert R.elem_err(ref + np.array([0, 0, 1e-30]), ref, np.abs(ref)) == float("inf")         # zero scale: exact
    assert R.elem_err(np.array([1.0, np.nan, 0.0]), ref, np.abs(ref)) == float("inf")
    assert R.elem_err(ref * (1 + 2 * R.U), ref, np.abs(ref)) <= 2 * R.U * (1 + 1e-9)


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------
def test_gpu_test_inputs_are_finite_in_the_reference():
    tab = R.coef_table()
    for kind in (0, 1):
        for n in R.LOSS_N:
            a, b = R.loss_inputs(kind, n)
            assert a.dtype == np.float32 and a.shape == (n,) and np.abs(a).max() <= (30 if kind else 2)
            if kind == 0:
                outs = [R.mse(a, b), R.mse_term_mag(a, b)] + [x for g in R.LOSS_G for x in R.mse_grad(a, b, g)]
            else:
                outs = [R.kl(a), R.kl_term_mag(a)] + [R.kl_grad(a, g) for g in R.LOSS_G] + \
                       [R.kl_grad_scale(a, g) for g in R.LOSS_G]
                held = [v for v in R.KL_SPECIALS if np.any((a == np.float32(v)) & (np.signbit(a) == np.signbit(v)))]
                assert len(held) == min(n, len(R.KL_SPECIALS)), (n, held)
            assert all(np.isfinite(o).all() for o in outs), (kind, n)
    for B, per in R.SCHED_SHAPES:
        a, b, g, t = R.sched_inputs(B, per)
        assert len(set(t.tolist())) == B and (B == 1 or {0, R.SCHED_T - 1} <= set(t.tolist()))
        outs = [R.q_sample(a, b, tab, t), R.predict_start(a, b, tab, t), R.q_sample_scale(a, b, tab, t),
                R.predict_start_scale(a, b, tab, t), *R.sched_backward(0, g, tab, t), *R.sched_backward(1, g, tab, t)]
        assert all(np.isfinite(o).all() for o in outs), (B, per)
    for B, C, HW in R.BN_SHAPES:
        x, w, b, rm, rv = R.bn_inputs(B, C, HW)
        assert rv.min() == np.float32(1e-6) and (C == 1 or rv.max() == np.float32(10.0))
        for name in R.ACT_NAMES:
            for wa in (w, None):
                for ba in (b, None):
                    assert np.isfinite(R.bn_eval(x, wa, ba, rm, rv, R.BN_EPS, name)).all()
                    assert np.isfinite(R.bn_eval_bar(x, wa, ba, rm, rv, R.BN_EPS, name)).all()
    for n in R.ACT_N:
        xs = R.act_inputs(n)
        allv = np.concatenate(xs)
        for v in R.ACT_SPECIALS:
            assert np.any((allv == np.float32(v)) & (np.signbit(allv) == np.signbit(v))), (n, v)
        for name in R.ACT_NAMES:
            assert all(x.shape == (n,) and np.isfinite(R.act_np(name, x)).all() for x in xs)
    for dim in R.EMBED_DIMS:
        assert np.isfinite(R.sinusoid(R.EMBED_T, dim)).all()


@pytest.mark.parametrize("name", R.CONV_BN_SHAPES)
def test_conv_bn_reference_against_modules(name):
    """The float64 conv -> frozen BN -> act restatement against nn.Conv2d / nn.ConvTranspose2d + nn.BatchNorm2d.eval()
    in float64 (values and all four gradients), on finite inputs whose BN holds the required entries."""
    from test_gpu_train import CONV_CASES
    case = CONV_CASES[name]
    B, Cin, H, W, Cout, k, s, p, op, tr, _a, has_bc, has_sk = case
    inp = R.conv_bn_inputs(case, 5)
    gamma, beta, mean, var = inp["bn"]
    assert gamma[0] < 0 and gamma[1] == 0 and var.min() == np.float32(1e-3) and var.max() == np.float32(4.0)
    assert (inp["bcast"] is not None) == has_bc and (inp["skip"] is not None) == has_sk
    conv = (torch.nn.ConvTranspose2d(Cin, Cout, k, s, p, output_padding=op) if tr
            else torch.nn.Conv2d(Cin, Cout, k, s, p)).double()
    bn = torch.nn.BatchNorm2d(Cout, eps=inp["eps"]).double().eval()
    with torch.no_grad():
        conv.weight.copy_(t64(inp["w"]))
        conv.bias.copy_(t64(inp["b"]))
        bn.weight.copy_(t64(gamma))
        bn.bias.copy_(t64(beta))
        bn.running_mean.copy_(t64(mean))
        bn.running_var.copy_(t64(var))
    for act_name in R.CONV_BN_ACTS:
        ref = R.conv_bn(case, inp, act_name)
        assert all(np.isfinite(v).all() for v in ref.values() if v is not None)
        conv.zero_grad()
        xt = t64(inp["x"]).requires_grad_()
        y = {"none": lambda v: v, "relu": torch.relu, "tanh": torch.tanh}[act_name](bn(conv(xt)))
        if has_bc:
            y = y + t64(inp["bcast"])[:, :, None, None]
        skt = t64(inp["skip"]).requires_grad_() if has_sk else None
        if has_sk:
            y = y + skt
        (y * t64(inp["R"])).sum().backward()
        assert close(ref["y"], y.detach(), 1e-11)
        assert close(ref["dx"], xt.grad, 1e-10) and close(ref["dw"], conv.weight.grad, 1e-10)
        assert close(ref["db"], conv.bias.grad, 1e-10)
        assert (ref["dskip"] is None) == (not has_sk) and (not has_sk or close(ref["dskip"], skt.grad))
