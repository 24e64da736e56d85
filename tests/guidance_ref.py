"""Float64 yardstick for style guidance.

Written from the definition: every step evaluates the denoiser under the target and under the base style on the same
x and t,
    e = e_b + s (e_t - e_b),
and e feeds the unchanged update: the reference's DDIM-style step with eta, or the multistep solver of
tests/solver_ref.py.  s is one strength per sample.  numpy only, except sample(), which calls the oracle's UNet
(oracle/ldm_torch_cpu.py) in float64, or tests/stylemix_ref.py's for stacked references.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as SR      # noqa: E402


def guide(e_t, e_b, s):
    """s: a number or one per sample ([B]), broadcast over the trailing dimensions."""
    e_t, e_b = np.asarray(e_t, dtype=np.float64), np.asarray(e_b, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    if s.ndim:
        s = s.reshape((-1,) + (1,) * (e_t.ndim - 1))
    return e_b + s * (e_t - e_b)


def ddim_step(ab, times, i, x, eps, eta):
    """The reference's update (model.py:442-458) from index times[i] to times[i + 1]; returns (x_next, x0)."""
    a_t, a_n = ab[times[i]], ab[times[i + 1]]
    x0 = (x - np.sqrt(1.0 - a_t) * eps) / np.sqrt(a_t)
    dxt, dxn = np.sqrt(1.0 - a_t) * eps, np.sqrt(1.0 - a_n) * eps
    return np.sqrt(a_n) * x0 + dxn + eta * (dxn - dxt), x0


def solve(ab, times, x, eps_t_fn, eps_b_fn, s, solver="dpmpp2m", eta=0.0):
    """The guided recursion; eps_*_fn(x, i) -> eps under the target / base.  solver "ddim" (with eta), "dpmpp1" or
    "dpmpp2m".  Returns (x_final, [x0_i], [eps_i]) with the guided x0 / eps."""
    order = {"ddim": 0, "dpmpp1": 1, "dpmpp2m": 2}[solver]
    x = np.asarray(x, dtype=np.float64)
    x0s, epss, prev = [], [], None
    for i in range(len(times) - 1):
        e = guide(eps_t_fn(x, i), eps_b_fn(x, i), s)
        if order:
            x, x0 = SR.step(ab, times, i, x, e, prev, order)
        else:
            x, x0 = ddim_step(ab, times, i, x, e, eta)
        x0s.append(x0)
        epss.append(e)
        prev = x0
    return x, x0s, epss


def plain(ab, times, x, eps_fn, solver="dpmpp2m", eta=0.0):
    """The unguided float64 loop, written without guide(): what s = 1 and s = 0 must reduce to."""
    order = {"ddim": 0, "dpmpp1": 1, "dpmpp2m": 2}[solver]
    if order:
        return SR.solve(ab, times, x, eps_fn, order)
    x = np.asarray(x, dtype=np.float64)
    x0s, epss = [], []
    for i in range(len(times) - 1):
        e = np.asarray(eps_fn(x, i), dtype=np.float64)
        x, x0 = ddim_step(ab, times, i, x, e, eta)
        x0s.append(x0)
        epss.append(e)
    return x, x0s, epss


def unet_eps_fn(sd64, times, B, s5, s6, key_w5=None, key_w6=None):
    """eps(x, i) of the oracle's UNet in float64 under the maps s5 / s6; with key weights (stacked references,
    stylemix_ref.key_weights) the weighted attention of tests/stylemix_ref.py."""
    import torch
    s5, s6 = torch.as_tensor(s5).double(), torch.as_tensor(s6).double()

    def fn(xv, i):
        with torch.no_grad():
            t = torch.full((B,), int(times[i]), dtype=torch.long)
            xt = torch.from_numpy(np.ascontiguousarray(xv))
            if key_w5 is None and key_w6 is None and s5.shape[2] * 4 == xt.shape[2]:   # one map per sample
                from oracle import ldm_torch_cpu as TC
                return TC.unet(sd64, xt, t, s5, s6).numpy()
            import stylemix_ref as MR
            return MR.unet(sd64, xt, t, s5, s6, key_w5, key_w6).numpy()

    return fn


def sample(sd64, ab, times, x, target, base, s, solver="dpmpp2m", eta=0.0):
    """target / base: (s5, s6) or (s5, s6, key_w5, key_w6)."""
    B = x.shape[0]
    return solve(ab, times, x, unet_eps_fn(sd64, times, B, *target), unet_eps_fn(sd64, times, B, *base), s, solver, eta)


def sample_plain(sd64, ab, times, x, maps, solver="dpmpp2m", eta=0.0):
    return plain(ab, times, x, unet_eps_fn(sd64, times, x.shape[0], *maps), solver, eta)
