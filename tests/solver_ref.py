"""Float64 yardstick for the multistep sampler (DPM-Solver++(2M) with a first-order first and last step).

Written from the solver's own lambda / h / r form,
    x_next = (sigma_next / sigma_t) x + alpha_next (1 - exp(-h)) D,    D = x0 + (x0 - x0_prev) / (2 r),
with D = x0 on a first-order step, independently of the {c_x, c_0, c_1} table the product evaluates.  numpy only,
except sample(), which calls the oracle's UNet (oracle/ldm_torch_cpu.py) in float64 for eps.
"""
import numpy as np


def alpha_bar(T=200):
    """The model's schedule in float64 from the fp32 table the model itself builds (beta = linspace(1e-4, 0.02, T))."""
    import torch
    beta = torch.linspace(0.0001, 0.02, T)
    return torch.cumprod(1 - beta, dim=0).double().numpy()


def sample_times(t_start, steps):
    """linspace(t_start, 0, steps + 1) truncated to integers, in float32 as torch.linspace computes it."""
    import torch
    return torch.linspace(t_start, 0, steps + 1).long().numpy()


def _sched(ab, t):
    a = ab[t]
    return np.sqrt(a), np.sqrt(1.0 - a), 0.5 * np.log(a / (1.0 - a))


def second_order(i, n, order=2):
    """Step i of n uses the history: never the first (none yet) nor the last (the jump to index 0)."""
    return order == 2 and 0 < i < n - 1


def step(ab, times, i, x, eps, x0_prev, order=2):
    """One step i -> i+1 on float64 arrays; returns (x_next, x0)."""
    n = len(times) - 1
    al_t, sg_t, lam_t = _sched(ab, times[i])
    al_n, sg_n, lam_n = _sched(ab, times[i + 1])
    h = lam_n - lam_t
    x0 = (x - sg_t * eps) / al_t
    D = x0
    if second_order(i, n, order):
        lam_p = _sched(ab, times[i - 1])[2]
        r = (lam_t - lam_p) / h
        D = x0 + (x0 - x0_prev) / (2.0 * r)
    return (sg_n / sg_t) * x + al_n * (-np.expm1(-h)) * D, x0


def coef_rows(ab, times, order=2):
    """The [n,8] table the product should hold, derived from step(): its response to unit x, x0 and x0_prev."""
    n = len(times) - 1
    out = np.zeros((n, 8))
    for i in range(n):
        al_t, sg_t, _ = _sched(ab, times[i])
        # x = 1 with eps chosen so that x0 = 0; then x0 = 1 with x = 0; then x0_prev = 1 alone
        cx = step(ab, times, i, np.float64(1.0), np.float64(1.0) / sg_t, np.float64(0.0), order)[0]
        c0 = step(ab, times, i, np.float64(0.0), -al_t / sg_t, np.float64(0.0), order)[0]
        c1 = step(ab, times, i, np.float64(0.0), np.float64(0.0), np.float64(1.0), order)[0]
        out[i] = [al_t, sg_t, cx, c0, c1, 0, 0, 0]
    return out


def solve(ab, times, x, eps_fn, order=2):
    """The whole recursion; eps_fn(x, i) -> eps.  Returns (x_final, [x0_i], [eps_i])."""
    x = np.asarray(x, dtype=np.float64)
    x0s, epss, prev = [], [], None
    for i in range(len(times) - 1):
        eps = np.asarray(eps_fn(x, i), dtype=np.float64)
        x, x0 = step(ab, times, i, x, eps, prev, order)
        x0s.append(x0)
        epss.append(eps)
        prev = x0
    return x, x0s, epss


def replay(ab, times, x, epss, order=2):
    """The recursion driven by recorded eps."""
    return solve(ab, times, x, lambda _x, i: epss[i], order)


def sample(sd64, ab, times, x, s5, s6, order=2):
    """The sampler with the oracle's UNet in float64 (sd64: the state dict as float64 tensors)."""
    import torch
    from oracle import ldm_torch_cpu as TC
    B = x.shape[0]
    s5, s6 = torch.as_tensor(s5).double(), torch.as_tensor(s6).double()

    def eps_fn(xv, i):
        with torch.no_grad():
            t = torch.full((B,), int(times[i]), dtype=torch.long)
            return TC.unet(sd64, torch.from_numpy(np.ascontiguousarray(xv)), t, s5, s6).numpy()

    return solve(ab, times, x, eps_fn, order)


# ---- the analytic model: Gaussian data N(0, s^2), eps*(x, t) = sigma_t x / (alpha_t^2 s^2 + sigma_t^2) ------------
S_DATA = 0.5


def gauss_eps(ab, t, x, s=S_DATA):
    al, sg, _ = _sched(ab, t)
    return sg * x / (al * al * s * s + sg * sg)


def gauss_exact(ab, t_from, t_to, x, s=S_DATA):
    """The probability-flow solution: x scales with the marginal's standard deviation."""
    a0, s0, _ = _sched(ab, t_from)
    a1, s1, _ = _sched(ab, t_to)
    return x * np.sqrt(a1 * a1 * s * s + s1 * s1) / np.sqrt(a0 * a0 * s * s + s0 * s0)


def table_solve(coef, x, eps_fn):
    """The product's form: drive a [n,8] coefficient table in float64; eps_fn(x, i)."""
    x = np.asarray(x, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    prev = None
    for i in range(coef.shape[0]):
        at, st, cx, c0, c1 = coef[i, :5]
        x0 = (x - st * eps_fn(x, i)) / at
        x = cx * x + c0 * x0 + (c1 * prev if prev is not None else 0.0)
        prev = x0
    return x
