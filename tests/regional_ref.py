"""Float64 yardstick for the regional keep.

Written from the definition: after every step's update (the reference's DDIM-style step with eta, or the multistep
solver of tests/solver_ref.py, on the plain or the guided noise prediction of tests/guidance_ref.py) the state is
blended with the content's own noising trajectory under a keep weight per sample and latent pixel,
    known = a_i z0 + b_i n0;   x_next = (1 - w) x_update + w known,
(a_i, b_i) = (sqrt(ab[t_i+1]), sqrt(1 - ab[t_i+1])), the last row (1, 0) with exact_last.  The logs and the solver's
history are the model's own x0 / eps, unblended.  numpy only, except sample(), which calls the oracle's UNet in float64
through guidance_ref.unet_eps_fn.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as GR    # noqa: E402
import solver_ref as SR      # noqa: E402


def keep_coefs(ab, times, exact_last=True):
    """[n, 2] float64 {sqrt(ab[t_i+1]), sqrt(1 - ab[t_i+1])}; with exact_last the last row is (1, 0)."""
    a_n = np.asarray(ab, dtype=np.float64)[np.asarray(times)[1:]]
    c = np.stack([np.sqrt(a_n), np.sqrt(1.0 - a_n)], 1)
    if exact_last and c.shape[0]:
        c[-1] = (1.0, 0.0)
    return c


def known(z0, n0, a, b):
    return a * np.asarray(z0, dtype=np.float64) + b * np.asarray(n0, dtype=np.float64)


def keep_blend(xu, z0, n0, w, a, b):
    """w [B, H, W] is shared by the channels of xu / z0 / n0 [B, C, H, W]."""
    w = np.asarray(w, dtype=np.float64)[:, None]
    return (1.0 - w) * np.asarray(xu, dtype=np.float64) + w * known(z0, n0, a, b)


def solve(ab, times, x, eps_fn, z0, n0, w, coefs, solver="dpmpp2m", eta=0.0, eps_b_fn=None, s=None):
    """The recursion with the keep; eps_b_fn / s: guided as in guidance_ref.solve.  Returns (x_final, [x0_i], [eps_i])
    with the unblended x0 / eps."""
    order = {"ddim": 0, "dpmpp1": 1, "dpmpp2m": 2}[solver]
    x = np.asarray(x, dtype=np.float64)
    x0s, epss, prev = [], [], None
    for i in range(len(times) - 1):
        e = np.asarray(eps_fn(x, i), dtype=np.float64)
        if eps_b_fn is not None:
            e = GR.guide(e, eps_b_fn(x, i), s)
        if order:
            xu, x0 = SR.step(ab, times, i, x, e, prev, order)
        else:
            xu, x0 = GR.ddim_step(ab, times, i, x, e, eta)
        x = keep_blend(xu, z0, n0, w, coefs[i][0], coefs[i][1])
        x0s.append(x0)
        epss.append(e)
        prev = x0
    return x, x0s, epss


def sample(sd64, ab, times, x, maps, z0, n0, w, solver="dpmpp2m", eta=0.0, base=None, s=None, exact_last=True):
    """maps / base: (s5, s6) or (s5, s6, key_w5, key_w6) as in guidance_ref.sample."""
    B = x.shape[0]
    fb = None if base is None else GR.unet_eps_fn(sd64, times, B, *base)
    return solve(ab, times, x, GR.unet_eps_fn(sd64, times, B, *maps), z0, n0, w, keep_coefs(ab, times, exact_last),
                 solver, eta, fb, s)
