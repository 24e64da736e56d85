"""Float64 yardstick for the train path's scalar kernels (csrc/misc.hip: losses, scheduler, eval BatchNorm,
activations, sinusoid) and for the frozen-BatchNorm conv (functional.conv(..., bn_eval=...)).

Written from the definitions, numpy float64 throughout; the activations and the conv restatement are float64 torch so
that autograd can differentiate them.  The module also holds the inputs both test files use (tests/test_train_ops_host.py
checks them on the CPU, tests/test_gpu_train_ops.py feeds them to the kernels) and the error measure the bars are
stated in:

    elem_err(y, ref, scale) = max_i |y_i - ref_i| / scale_i

with scale_i the magnitude of the operands that were rounded on the way to element i, so an error confined to small
elements is not hidden behind the largest one.  U = 2^-24 is fp32's unit roundoff; a bar of k U allows k/2 roundings
of operands of that magnitude (factor 2 margin), fused multiply-add or not.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
KL_EPS = 1e-8


def f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def elem_err(y, ref, scale):
    """max_i |y_i - ref_i| / scale_i.  Where scale_i is 0 the element must be exact; a NaN anywhere is inf."""
    y, ref = f64(y), f64(ref)
    scale = np.broadcast_to(f64(scale), ref.shape)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    d = np.abs(y - ref)
    if not (np.isfinite(d).all() and np.isfinite(scale).all()):
        return float("inf")
    if d.size == 0:
        return 0.0
    zero = scale == 0
    if (d[zero] != 0).any():
        return float("inf")
    return float((d[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def uniform(shape, seed, lo=-1.0, hi=1.0):
    return rng(seed).uniform(lo, hi, shape).astype(np.float32)


# ---- losses -----------------------------------------------------------------------------------------
def mse(a, b):
    a, b = f64(a), f64(b)
    return float(np.mean((a - b) ** 2))


def kl(a):
    a = f64(a)
    return float(np.mean(0.5 * (a * a - 1.0 - np.log(a * a + KL_EPS))))


def mse_term_mag(a, b):
    """Magnitude of one term of the MSE sum as the kernel forms it."""
    return (f64(a) - f64(b)) ** 2


def kl_term_mag(a):
    a = f64(a)
    return 0.5 * (a * a + 1.0 + np.abs(np.log(a * a + KL_EPS)))


def loss_bar(ref, term_mag):
    """|loss - ref| allowed: the per-term fp32 arithmetic (the partial sums are fp64) and the final cast."""
    return 8 * U * float(np.mean(term_mag)) + U * abs(ref)


def mse_grad(a, b, g):
    """(ga, gb) of g * mean((a-b)^2)."""
    a, b = f64(a), f64(b)
    ga = 2.0 * (a - b) * float(g) / a.size
    return ga, -ga


def kl_grad(a, g):
    a = f64(a)
    return float(g) * (a - a / (a * a + KL_EPS)) / a.size


def kl_grad_scale(a, g):
    """Magnitude of the two operands of the KL gradient's subtraction (they cancel near |a| = 1)."""
    a = f64(a)
    return (np.abs(a) + np.abs(a / (a * a + KL_EPS))) * abs(float(g)) / a.size


KL_SPECIALS = (0.0, -0.0, 1e-5, -1e-5, 1e-4, -1e-4, 1.0, -1.0, 30.0, -30.0)
LOSS_N = (1, 63, 255, 256, 257, 131072, 131073, 300001)
LOSS_G = (1.0, 0.37, 65536.0)


def loss_inputs(kind, n):
    """(a, b) float32: uniform in [-2, 2]; for KL (kind 1, b None) fixed positions hold KL_SPECIALS."""
    a = uniform((n,), 100 + kind, -2.0, 2.0)
    if kind == 0:
        return a, uniform((n,), 102, -2.0, 2.0)
    for i, v in enumerate(KL_SPECIALS):
        pos = i * n // len(KL_SPECIALS) if n >= len(KL_SPECIALS) else i
        if pos < n:
            a[pos] = v
    return a, None


# ---- scheduler --------------------------------------------------------------------------------------
SCHED_T = 200
SCHED_SHAPES = ((1, 1), (5, 7), (5, 257), (3, 1000), (4, 255))


def coef_table(T=SCHED_T):
    """[T, 2] float32 {sqrt(ab), sqrt(1 - ab)} of the linear beta schedule 1e-4 .. 0.02."""
    ab = np.cumprod(1.0 - np.linspace(1e-4, 0.02, T))
    return np.stack([np.sqrt(ab), np.sqrt(1.0 - ab)], axis=1).astype(np.float32)


def sched_t(B, T=SCHED_T):
    """Distinct timesteps, one per sample, with 0 and T - 1 among them (B = 1: T - 1)."""
    if B == 1:
        return np.array([T - 1], dtype=np.int64)
    mid = rng(7).permutation(np.arange(1, T - 1))[:B - 2]
    return np.concatenate([[T - 1], mid, [0]]).astype(np.int64)


def sched_inputs(B, per):
    """(first, second, upstream gradient) float32 [B, per], t int64 [B]."""
    return (uniform((B, per), 200, -2, 2), uniform((B, per), 201, -2, 2), uniform((B, per), 202, -2, 2),
            sched_t(B))


def _coef(table, t, ndim):
    """Per-sample (sa, s1) float64 from the float32 table, shaped to broadcast; an out-of-range t gives NaN."""
    tab = f64(table)
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    ok = (t >= 0) & (t < tab.shape[0])
    rows = tab[np.where(ok, t, 0)]
    rows = np.where(ok[:, None], rows, np.nan)
    shp = (-1,) + (1,) * (ndim - 1)
    return rows[:, 0].reshape(shp), rows[:, 1].reshape(shp)


def q_sample(x0, eps, table, t):
    x0, eps = f64(x0), f64(eps)
    sa, s1 = _coef(table, t, x0.ndim)
    return sa * x0 + s1 * eps


def q_sample_scale(x0, eps, table, t):
    x0, eps = f64(x0), f64(eps)
    sa, s1 = _coef(table, t, x0.ndim)
    return np.abs(sa * x0) + np.abs(s1 * eps) + np.abs(sa * x0 + s1 * eps)


def predict_start(zt, eps, table, t):
    zt, eps = f64(zt), f64(eps)
    sa, s1 = _coef(table, t, zt.ndim)
    return (zt - s1 * eps) / sa


def predict_start_scale(zt, eps, table, t):
    zt, eps = f64(zt), f64(eps)
    sa, s1 = _coef(table, t, zt.ndim)
    return (np.abs(zt) + np.abs(s1 * eps)) / sa


def sched_backward(kind, g, table, t):
    """(ga, gb): kind 0 of q_sample (sa g, s1 g), kind 1 of predict_start (g / sa, -s1 g / sa)."""
    g = f64(g)
    sa, s1 = _coef(table, t, g.ndim)
    if kind == 0:
        return sa * g, s1 * g
    return g / sa, -(s1 * g) / sa


# ---- activations (float64 torch: differentiable) ------------------------------------------------------
ACT_NAMES = ("none", "relu", "tanh", "tanh_half", "gelu")
ACT_EXACT = ("none", "relu")          # no rounding at all: the kernel's output is the input or 0
ACT_LIPSCHITZ = {"none": 1.0, "relu": 1.0, "tanh": 1.0, "tanh_half": 0.5, "gelu": 1.13}   # max |act'|


def act(name, v):
    """v: float64 torch tensor."""
    if name == "none":
        return v
    if name == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if name == "tanh":
        return torch.tanh(v)
    if name == "tanh_half":
        return (torch.tanh(v) + 1.0) / 2.0
    if name == "gelu":
        return v * 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
    raise KeyError(name)


def act_np(name, v):
    return act(name, torch.from_numpy(np.ascontiguousarray(f64(v)))).numpy()


def act_bar(name, ref):
    """Absolute error allowed per element for sinf / cosf / tanhf / expf / erff (documented at a few ulp): 1e-6 for
    outputs bounded by 1, 1e-6 max(1, |ref|) otherwise; 0 for the activations that round nothing."""
    ref = f64(ref)
    if name in ACT_EXACT:
        return np.zeros_like(ref)
    if name in ("tanh", "tanh_half"):
        return np.full_like(ref, 1e-6)
    return 1e-6 * np.maximum(1.0, np.abs(ref))


ACT_SPECIALS = (0.0, -0.0, 1e-8, -1e-8, 0.5, -0.5, 6.0, -6.0, 20.0, -20.0)
ACT_N = (1, 255, 257)


def act_inputs(n):
    """List of float32 vectors of n elements which together hold every ACT_SPECIALS value: one vector with the
    specials spread over uniform [-4, 4] values, or (n smaller than the list) one vector per special."""
    k = len(ACT_SPECIALS)
    if n < k:
        return [np.full((n,), v, dtype=np.float32) for v in ACT_SPECIALS]
    x = uniform((n,), 300, -4, 4)
    for i, v in enumerate(ACT_SPECIALS):
        x[i * n // k] = v
    return [x]


# ---- eval BatchNorm -----------------------------------------------------------------------------------
BN_SHAPES = ((1, 1, 1), (2, 3, 63), (3, 5, 64), (2, 16, 257))
BN_EPS = 1e-5


def bn_inputs(B, C, HW):
    """x [B, C, HW], weight, bias, running_mean, running_var [C] float32; the variances span 1e-6 .. 10."""
    rv = np.geomspace(1e-6, 10.0, C) if C > 1 else np.array([1e-6])
    return (uniform((B, C, HW), 400, -2, 2), uniform((C,), 401, -1.5, 1.5), uniform((C,), 402, -0.5, 0.5),
            uniform((C,), 403, -0.5, 0.5), rv.astype(np.float32))


def _bn_affine(x, w, b, rm, rv, eps):
    x = f64(x)
    shp = (1, -1) + (1,) * (x.ndim - 2)
    one = np.ones(x.shape[1])
    alpha = (one if w is None else f64(w)) / np.sqrt(f64(rv) + float(eps))
    beta = (0.0 * one if b is None else f64(b)) - f64(rm) * alpha
    return x, alpha.reshape(shp), beta.reshape(shp), (f64(rm) * alpha).reshape(shp)


def bn_eval(x, w, b, rm, rv, eps, act_name="none"):
    """act((x - rm) / sqrt(rv + eps) * w + b) for x [B, C, ...]; w / b None = 1 / 0."""
    x, alpha, beta, _ = _bn_affine(x, w, b, rm, rv, eps)
    return act_np(act_name, x * alpha + beta)


def bn_eval_scale(x, w, b, rm, rv, eps):
    """|x alpha| + |beta| + |rm alpha| with alpha = w / sqrt(rv + eps), beta = b - rm alpha."""
    x, alpha, beta, rma = _bn_affine(x, w, b, rm, rv, eps)
    return np.abs(x * alpha) + np.abs(beta) + np.abs(rma)


def bn_eval_bar(x, w, b, rm, rv, eps, act_name):
    """Absolute error allowed per element: 8 U of the affine part's operands, carried through the activation (at most
    max |act'| times as large), plus the activation's own bar."""
    pre = bn_eval_scale(x, w, b, rm, rv, eps)
    return ACT_LIPSCHITZ[act_name] * 8 * U * pre + act_bar(act_name, bn_eval(x, w, b, rm, rv, eps, act_name))


# ---- time embedding -------------------------------------------------------------------------------------
EMBED_DIMS = (8, 128)
EMBED_T = (0, 1, 17, 199, 999)


def sinusoid_freqs(dim):
    """The model's float32 table exp(arange(half) * -(ln 1e4 / (half - 1))), formed in float32 as the model forms it."""
    half = dim // 2
    e = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half) * -e).to(torch.float32).numpy()


def sinusoid(t, dim):
    """[len(t), dim] = sin | cos of float32(t) * float32(freq), the product rounded once to float32 (as the kernel and
    the model form the argument), the functions in float64."""
    tv = np.asarray(t).astype(np.float32).reshape(-1)
    arg = (tv[:, None] * sinusoid_freqs(dim)[None, :]).astype(np.float32).astype(np.float64)
    return np.concatenate([np.sin(arg), np.cos(arg)], axis=1)


# ---- conv with a frozen eval-mode BatchNorm in its epilogue ---------------------------------------------------
# names of tests/test_gpu_train.py CONV_CASES: stride 1, stride 2 (+bcast), convT with skip, 1x1, Cin = 1
CONV_BN_SHAPES = ("unet_enc1_k3s1", "unet_enc2_k3s2_temb", "unet_dec2_convT_skip", "proj_1x1", "style_enc1_cin1")
CONV_BN_ACTS = ("none", "relu", "tanh")


def conv_bn_inputs(case, seed):
    """case: a CONV_CASES tuple.  float32 arrays x, w, b, the BN's (gamma, beta, mean, var), eps, bcast / skip (or
    None) and the upstream gradient R.  The variances span 1e-3 .. 4; gamma has a negative and a zero entry
    (one entry, negative, when Cout = 1)."""
    import torch.nn.functional as tF
    B, Cin, H, W, Cout, k, s, p, op, tr, _act, has_bc, has_sk = case
    x = uniform((B, Cin, H, W), seed)
    w = uniform((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), seed + 1, -0.2, 0.2)
    b = uniform((Cout,), seed + 2, -0.1, 0.1)
    gamma = uniform((Cout,), seed + 6, 0.5, 1.5)
    gamma[0] = -gamma[0]
    if Cout > 1:
        gamma[1] = 0.0
    beta = uniform((Cout,), seed + 7, -0.1, 0.1)
    mean = uniform((Cout,), seed + 8, -0.2, 0.2)
    var = rng(seed + 9).permutation(np.geomspace(1e-3, 4.0, Cout) if Cout > 1 else np.array([1e-3])).astype(np.float32)
    xt, wt = torch.zeros((B, Cin, H, W)), torch.from_numpy(w)
    oshape = tuple((tF.conv_transpose2d(xt, wt, None, stride=s, padding=p, output_padding=op) if tr
                    else tF.conv2d(xt, wt, None, stride=s, padding=p)).shape)
    bc = uniform((B, Cout), seed + 3) if has_bc else None
    sk = uniform(oshape, seed + 4) if has_sk else None
    R = uniform(oshape, seed + 5)
    return dict(x=x, w=w, b=b, bn=(gamma, beta, mean, var), eps=BN_EPS, bcast=bc, skip=sk, R=R)


def conv_bn(case, inp, act_name):
    """float64: conv -> (v - rm) / sqrt(rv + eps) * w + b -> act (+bcast) (+skip), and the gradients of sum(y R).
    Returns dict y, dx, dw, db, dskip (None without a skip)."""
    import torch.nn.functional as tF
    _B, _Cin, _H, _W, _Cout, _k, s, p, op, tr = case[:10]
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()   # noqa: E731
    xt, wt, bt = (t64(inp[k]).requires_grad_() for k in ("x", "w", "b"))
    if tr:
        v = tF.conv_transpose2d(xt, wt, bt, stride=s, padding=p, output_padding=op)
    else:
        v = tF.conv2d(xt, wt, bt, stride=s, padding=p)
    g, be, rm, rv = (t64(a)[None, :, None, None] for a in inp["bn"])
    y = act(act_name, (v - rm) / torch.sqrt(rv + inp["eps"]) * g + be)
    if inp["bcast"] is not None:
        y = y + t64(inp["bcast"])[:, :, None, None]
    skt = None
    if inp["skip"] is not None:
        skt = t64(inp["skip"]).requires_grad_()
        y = y + skt
    (y * t64(inp["R"])).sum().backward()
    return dict(y=y.detach().numpy(), dx=xt.grad.numpy(), dw=wt.grad.numpy(), db=bt.grad.numpy(),
                dskip=None if skt is None else skt.grad.numpy())
