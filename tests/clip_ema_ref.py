"""numpy float64 restatement of gradient-norm clipping, clipped Adam / AdamW and the EMA of the weights
(ldm_amd.optim: ldm_unscale_check_norm + ldm_grad_norm_finalize, ldm_adam_step_ext, ldm_ema_update).

Definitions (torch.nn.utils.clip_grad_norm_, torch.optim.Adam / AdamW, the usual EMA):
  norm  = sqrt(sum over all tensors of sum g^2)
  coef  = min(1, max_norm / (norm + 1e-6))        (max_norm <= 0: norm only, coef = 1)
  g'    = g * coef
  Adam  : g' += wd * p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;
          p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
  AdamW : p *= 1 - lr * wd first, no L2 term
  EMA   : e += (1 - decay) * (p_new - e)
"""
import numpy as np

# the tensor set of the tests: every path of the chunk map (4096 elements per chunk) and of chunk_for in one table
#   1, 3: tail only; 4096: exactly one chunk; 4097: a chunk plus a one-element tail chunk; 4098; 12289: several
#   chunks; (7, 5); "offset": a contiguous view one element into its storage (not 16-byte aligned: scalar path)
SHAPES = [(1,), (3,), (4096,), (4097,), (4098,), (12289,), (7, 5), (1001,)]
OFFSET_INDEX = 7      # SHAPES[7] is the view at a storage offset of one element
BIG_INDEX = 5         # this tensor's gradients are 1e3 times larger than the rest, so clipping bites


def tensors(seed, scale=1.0):
    """One fp32 array per shape, standard normal x scale, fixed seed."""
    g = np.random.Generator(np.random.PCG64(seed))
    return [(g.standard_normal(s) * scale).astype(np.float32) for s in SHAPES]


def grads(seed):
    gs = tensors(seed, 1e-2)
    gs[BIG_INDEX] = (gs[BIG_INDEX].astype(np.float64) * 1e3).astype(np.float32)
    return gs


def grad_norm(gs):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in gs)))


def clip_coef(norm, max_norm):
    if max_norm <= 0:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if (c != c or c < 1.0) else 1.0     # NaN stays NaN, as torch's clamp(max=1) leaves it


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, coef=1.0):
    """One (clipped) Adam / AdamW step in float64; returns (p, m, v)."""
    b1, b2 = betas
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g * coef
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    elif weight_decay != 0.0:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** step) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v


def ema_step(e, p_new, decay):
    e = np.asarray(e, dtype=np.float64)
    return e + (1.0 - decay) * (np.asarray(p_new, dtype=np.float64) - e)


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between two fp32 values of the same sign."""
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return 0
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))
