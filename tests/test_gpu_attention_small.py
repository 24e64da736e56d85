"""The LDS-resident cross-attention kernels (L, S <= 64) over ragged and unequal L, S, kernel by kernel.

csrc/misc.hip: attention_mfma_kernel (plain, folded-query and probabilities-only instances, chosen by
L <= LP && S <= SP with pads 16 / 32 / 64) and the VALU fallback attention_core_kernel (head dims without an
MFMA instance); csrc/backward.hip: attention_backward_mfma_kernel (L, S, d multiples of 16) and the scalar
attention_backward_kernel; and the shapes within 64 tokens that the resident backward cannot hold (d = 128,
47 - 63 tokens that are no multiple of 16), which functional.attention_core sends to the KV-tiled pair of flash.hip.

Reference: float64 torch of softmax((q * scale)^T k) v per head, float64 autograd for the gradients.  heads = 4 and
B = 3 everywhere.  Metric: conftest.rel_err (1e-4 forward and gradients, 1e-5 folded form and probabilities), and the
same bound per token row (max error over the head's channels of one token against max |ref| there), so that one bad
masked row cannot hide under a large element elsewhere.  fp32 CPU torch of the same formulas stays inside every
per-row bound on these inputs (worst row: 1.5e-6 forward, 4.1e-6 gradients, 1.6e-6 folded form, 1.4e-6
probabilities), so none is widened.  The softmax-range cases at the end carry their own measured bounds.

Every raw call writes into the middle of a larger tensor: the payload pre-filled with NaN must come back finite, and
the 64-float guard bands on both sides must keep their sentinel bits (stray writes of masked lanes / idle blocks).
"""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

HEADS, B = 4, 3
TOL, TOL_FOLD = 1e-4, 1e-5
GUARD = 64                    # floats; a multiple of 4, so the payload keeps the allocation's 16-byte alignment
SENTINEL = -1234.5678


def npy(t):
    return t.detach().double().cpu().numpy()


# ---- the formulas, in the dtype of their inputs (float64: the reference; float32 on the CPU: the bounds' check) ----
def attn(q, kv):
    """softmax((q*scale)^T k) v per head; q [B,E,L], kv [B,2E,S] channel-major -> [B,E,L]."""
    Bn, E, L = q.shape
    S, d = kv.shape[2], E // HEADS
    qh = q.reshape(Bn, HEADS, d, L).transpose(2, 3) * math.sqrt(1.0 / d)       # [B,h,L,d]
    k = kv[:, :E].reshape(Bn, HEADS, d, S)
    v = kv[:, E:].reshape(Bn, HEADS, d, S)
    p = torch.softmax(qh @ k, -1)                                              # [B,h,L,S]
    return (v @ p.transpose(2, 3)).reshape(Bn, E, L)


def folded_probs(z, kv, wq, bq):
    """P [B,h,L,S] of the attention whose queries are Wq z + bq; z [B,L,E] token-major."""
    Bn, L, E = z.shape
    S, d = kv.shape[2], E // HEADS
    q = torch.einsum("oe,ble->blo", wq, z) + bq
    qh = q.view(Bn, L, HEADS, d).permute(0, 2, 1, 3) * math.sqrt(1.0 / d)      # [B,h,L,d]
    return torch.softmax(qh @ kv[:, :E].reshape(Bn, HEADS, d, S), -1)


def folded(z, kv, wq, bq):
    """-> [B,L,E] token-major."""
    Bn, L, E = z.shape
    S, d = kv.shape[2], E // HEADS
    p = folded_probs(z, kv, wq, bq)
    v = kv[:, E:].reshape(Bn, HEADS, d, S)
    return torch.einsum("bhls,bhds->blhd", p, v).reshape(Bn, L, E)


def logits64(q, kv):
    Bn, E, L = q.shape
    S, d = kv.shape[2], E // HEADS
    qh = q.double().reshape(Bn, HEADS, d, L).transpose(2, 3) * math.sqrt(1.0 / d)
    return qh @ kv.double()[:, :E].reshape(Bn, HEADS, d, S)


def grads(q, kv, dout):
    """(y, dq, dkv) by autograd in the dtype of the inputs."""
    q, kv = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    y = attn(q, kv)
    (y * dout).sum().backward()
    return y.detach(), q.grad, kv.grad


# ---- metrics ---------------------------------------------------------------------------------------
def row_err(y, ref, layout):
    """max over token rows of (max error over the head's channels / max |ref| over them).  layout "cm": [B,E,T]
    channel-major, "tm": [B,T,E] token-major, "p": [B,h,L,S] (a row = one query's probabilities)."""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if layout == "cm":
        shp, ax = (y.shape[0], HEADS, y.shape[1] // HEADS, y.shape[2]), 2
    elif layout == "tm":
        shp, ax = (y.shape[0], y.shape[1], HEADS, y.shape[2] // HEADS), 3
    else:
        shp, ax = y.shape, 3
    y, ref = y.reshape(shp), ref.reshape(shp)
    return float((np.abs(y - ref).max(axis=ax) / np.maximum(np.abs(ref).max(axis=ax), 1e-30)).max())


def check(y, ref, tol, layout, what, row_tol=None):
    e, er = rel_err(npy(y), npy(ref)), row_err(npy(y), npy(ref), layout)
    print(f"{what}: rel_err {e:.3e} (<= {tol:.1e}), worst row {er:.3e} (<= {tol if row_tol is None else row_tol:.1e})")
    assert e <= tol, what
    assert er <= (tol if row_tol is None else row_tol), what + " (per row)"


# ---- guarded outputs ---------------------------------------------------------------------------------
class Guarded:
    """A NaN-filled payload of `shape` between two sentinel guard bands of one tensor."""

    def __init__(self, shape, dev):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(float("nan"))
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        want = torch.full((GUARD,), SENTINEL).view(torch.int32)
        lo, hi = self.buf[:GUARD].cpu().view(torch.int32), self.buf[GUARD + self.n:].cpu().view(torch.int32)
        return torch.equal(lo, want) and torch.equal(hi, want)

    def written(self):
        """the payload, after checking that every element was written and nothing beside it"""
        torch.cuda.synchronize()
        assert self.guards_intact(), "a guard band was written"
        assert torch.isfinite(self.t).all(), "an output element was left unwritten (or is not finite)"
        return self.t

    def untouched(self):
        torch.cuda.synchronize()
        assert self.guards_intact(), "a guard band was written"
        assert torch.isnan(self.t).all(), "a failed call wrote output"


def stream():
    return torch.cuda.current_stream().cuda_stream


def scale_of(E):
    return float(math.sqrt(1.0 / float(E // HEADS)))


# ---- inputs and float64 references, computed once per shape -------------------------------------------
@functools.lru_cache(maxsize=None)
def case(E, L, S):
    g = torch.Generator().manual_seed(1000 * E + 64 * L + S)
    q = torch.randn(B, E, L, generator=g)
    kv = torch.randn(B, 2 * E, S, generator=g)
    dout = torch.randn(B, E, L, generator=g)
    y, dq, dkv = grads(q.double(), kv.double(), dout.double())
    return {"q": q, "kv": kv, "dout": dout, "y": y, "dq": dq, "dkv": dkv}


@functools.lru_cache(maxsize=None)
def fold_case(E, L, S):
    g = torch.Generator().manual_seed(7 * E + 64 * L + S)
    c = {"z": torch.randn(B, L, E, generator=g), "kv": torch.randn(B, 2 * E, S, generator=g),
         "wq": torch.randn(E, E, generator=g) / E ** 0.5, "bq": torch.randn(E, generator=g) * 0.1}
    args = [c[k].double() for k in ("z", "kv", "wq", "bq")]
    c["y"], c["p"] = folded(*args), folded_probs(*args)
    return c


# ---- raw calls ---------------------------------------------------------------------------------------
def raw_forward(cuda, q, kv):
    from ldm_amd import _lib as Lb
    Bn, E, L = q.shape
    out = Guarded((Bn, E, L), cuda)
    qd, kvd = q.to(cuda), kv.to(cuda)
    Lb.call("ldm_attention_core", qd.data_ptr(), kvd.data_ptr(), out.ptr(), Bn, E, HEADS, L, kv.shape[2], scale_of(E),
            stream())
    return out.written()


def raw_fold_keys(cuda, c):
    from ldm_amd import _lib as Lb
    E, S = c["wq"].shape[0], c["kv"].shape[2]
    dv = {k: c[k].to(cuda) for k in ("z", "kv", "wq", "bq")}
    kf = Guarded((B, HEADS, S, E), cuda)
    bf = Guarded((B, HEADS, S), cuda)
    Lb.call("ldm_attention_fold_keys", dv["kv"].data_ptr(), dv["wq"].data_ptr(), dv["bq"].data_ptr(), B, E, HEADS, S,
            scale_of(E), kf.ptr(), bf.ptr(), stream())
    return dv, kf.written(), bf.written()


def raw_folded(cuda, c):
    from ldm_amd import _lib as Lb
    L, E = c["z"].shape[1:]
    dv, kf, bf = raw_fold_keys(cuda, c)
    out = Guarded((B, L, E), cuda)
    Lb.call("ldm_attention_folded", dv["z"].data_ptr(), dv["kv"].data_ptr(), kf.data_ptr(), bf.data_ptr(), out.ptr(), B,
            E, HEADS, L, c["kv"].shape[2], stream())
    return out.written()


def raw_backward(cuda, q, kv, dout, flash):
    """(dq, dkv) of the LDS-resident entry point, or of the KV-tiled pair (forward with lse, then backward)."""
    from ldm_amd import _lib as Lb
    Bn, E, L = q.shape
    S = kv.shape[2]
    qd, kvd, dd = q.to(cuda), kv.to(cuda), dout.to(cuda)
    dq, dkv = Guarded((Bn, E, L), cuda), Guarded((Bn, 2 * E, S), cuda)
    if flash:
        out, lse, delta = Guarded((Bn, E, L), cuda), Guarded((Bn, HEADS, L), cuda), Guarded((Bn, HEADS, L), cuda)
        Lb.call("ldm_attention_forward_lse", qd.data_ptr(), kvd.data_ptr(), out.ptr(), lse.ptr(), Bn, E, HEADS, L, S,
                scale_of(E), stream())
        Lb.call("ldm_attention_backward_flash", qd.data_ptr(), kvd.data_ptr(), out.written().data_ptr(),
                lse.written().data_ptr(), dd.data_ptr(), dq.ptr(), dkv.ptr(), delta.ptr(), Bn, E, HEADS, L, S,
                scale_of(E), stream())
        delta.written()
    else:
        Lb.call("ldm_attention_backward", qd.data_ptr(), kvd.data_ptr(), dd.data_ptr(), dq.ptr(), dkv.ptr(), Bn, E,
                HEADS, L, S, scale_of(E), stream())
    return dq.written(), dkv.written()


# ---- a. forward, channel-major -------------------------------------------------------------------------
MFMA_LS = [(1, 1), (3, 16), (16, 3), (5, 13), (16, 17), (17, 16), (24, 32), (32, 24), (33, 9), (9, 33), (40, 64),
           (64, 40), (50, 50), (63, 63), (64, 64)]
FWD = ([(E, L, S) for E in (256, 512) for (L, S) in MFMA_LS] +
       [(128, 16, 48), (128, 64, 64), (128, 80, 40),   # d = 32: no MFMA instance, the VALU fallback
        (96, 20, 36)])                                  # d = 24


@pytest.mark.parametrize("E,L,S", FWD)
def test_forward(cuda, E, L, S):
    from ldm_amd import ops
    c = case(E, L, S)
    assert not ops.attention_uses_flash(E, HEADS, L, S)
    out = raw_forward(cuda, c["q"], c["kv"])
    check(out, c["y"], TOL, "cm", f"forward E={E} L={L} S={S}")
    out2 = ops.attention_core(c["q"].to(cuda), c["kv"].to(cuda), HEADS)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


@pytest.mark.parametrize("E", [256, 512])
def test_forward_hands_over_past_64(cuda, E):
    """The resident instances end at 64 tokens on either side; one more goes to the KV-tiled kernel, same result."""
    from ldm_amd import ops
    assert not ops.attention_uses_flash(E, HEADS, 64, 64)
    for L, S in ((65, 64), (64, 65)):
        assert ops.attention_uses_flash(E, HEADS, L, S)
        c = case(E, L, S)
        out = raw_forward(cuda, c["q"], c["kv"])
        check(out, c["y"], TOL, "cm", f"forward E={E} L={L} S={S}")
        assert torch.equal(out, ops.attention_core(c["q"].to(cuda), c["kv"].to(cuda), HEADS))


# ---- b. backward ---------------------------------------------------------------------------------------
BWD_MFMA = [(256, 16, 48), (256, 64, 16), (256, 32, 32), (256, 48, 64), (512, 16, 16), (512, 32, 64), (512, 64, 64),
            (128, 16, 32), (128, 64, 64)]
# (512, 46, 46): 64 032 B of LDS, the largest equal-sided shape the scalar form holds at d = 128
BWD_SCALAR = [(256, 5, 13), (256, 17, 16), (256, 40, 24), (256, 63, 63), (512, 36, 20), (512, 46, 46), (96, 20, 36)]
# beyond the scalar form's 64 KiB and no multiple of 16: these raised "head tile exceeds LDS budget" in backward()
# before functional.attention_core routed them to the KV-tiled pair
BWD_FLASH = [(512, 47, 47), (512, 50, 50), (512, 63, 63), (512, 64, 50), (512, 50, 64)]
BWD = [(E, L, S, "mfma") for E, L, S in BWD_MFMA] + [(E, L, S, "scalar") for E, L, S in BWD_SCALAR] + \
      [(E, L, S, "flash") for E, L, S in BWD_FLASH]


def check_grads(y, dq, dkv, c, E, what, tol=None, row=None):
    tol, row = tol or {}, row or {}
    for name, got, ref in (("y", y, c["y"]), ("dq", dq, c["dq"]), ("dK", dkv[:, :E], c["dkv"][:, :E]),
                           ("dV", dkv[:, E:], c["dkv"][:, E:])):
        check(got, ref, tol.get(name, TOL), "cm", f"{what} {name}", row.get(name, TOL))


def autograd_backward(cuda, c):
    from ldm_amd import functional as HF
    qd, kvd = c["q"].to(cuda).requires_grad_(True), c["kv"].to(cuda).requires_grad_(True)
    y = HF.attention_core(qd, kvd, HEADS)
    (y * c["dout"].to(cuda)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), qd.grad, kvd.grad


@pytest.mark.parametrize("E,L,S,form", BWD)
def test_backward(cuda, E, L, S, form):
    from ldm_amd import ops
    c = case(E, L, S)
    assert ops.attention_backward_uses_flash(E, HEADS, L, S) == (form == "flash")
    y, dq, dkv = autograd_backward(cuda, c)
    check_grads(y, dq, dkv, c, E, f"backward ({form}) E={E} L={L} S={S}")
    # the same kernels through their C entry points, into guarded outputs: the same bits, and nothing beside them
    rdq, rdkv = raw_backward(cuda, c["q"], c["kv"], c["dout"], form == "flash")
    assert torch.equal(rdq, dq) and torch.equal(rdkv, dkv)


@pytest.mark.parametrize("E,L,S,form", BWD)
def test_backward_supported_predicts_the_dispatch(cuda, E, L, S, form):
    """ldm_attention_backward_supported is 1 exactly where ldm_attention_backward runs; where it is 0 the entry point
    fails cleanly (the LDS-budget error) and writes nothing."""
    from ldm_amd import _lib as Lb
    lib = Lb.load()
    c = case(E, L, S)
    assert lib.ldm_attention_backward_supported(E, HEADS, L, S) == (0 if form == "flash" else 1)
    qd, kvd, dd = c["q"].to(cuda), c["kv"].to(cuda), c["dout"].to(cuda)
    dq, dkv = Guarded((B, E, L), cuda), Guarded((B, 2 * E, S), cuda)
    rc = lib.ldm_attention_backward(qd.data_ptr(), kvd.data_ptr(), dd.data_ptr(), dq.ptr(), dkv.ptr(), B, E, HEADS, L, S,
                                    scale_of(E), stream())
    if form == "flash":
        assert rc != 0 and b"LDS budget" in lib.ldm_last_error()
        dq.untouched()
        dkv.untouched()
    else:
        assert rc == 0
        dq.written()
        dkv.written()


# ---- c. folded forward ---------------------------------------------------------------------------------
FOLD = [(256, 5, 13), (256, 10, 10), (256, 24, 24), (256, 40, 40), (256, 48, 64), (256, 64, 40),
        (512, 4, 4), (512, 10, 10), (512, 12, 16), (512, 16, 12), (512, 24, 24), (512, 32, 20)]


@pytest.mark.parametrize("E,L,S", FOLD)
def test_folded(cuda, E, L, S):
    c = fold_case(E, L, S)
    check(raw_folded(cuda, c), c["y"], TOL_FOLD, "tm", f"folded E={E} L={L} S={S}")


def test_folded_without_an_instance_fails_cleanly(cuda):
    """E = 512 has folded instances up to 32 x 32: 33 x 33 must be an error, not a launch."""
    from ldm_amd import _lib as Lb
    E, L, S = 512, 33, 33
    c = fold_case(E, L, S)
    dv, kf, bf = raw_fold_keys(cuda, c)
    out = Guarded((B, L, E), cuda)
    args = (dv["z"].data_ptr(), dv["kv"].data_ptr(), kf.data_ptr(), bf.data_ptr(), out.ptr(), B, E, HEADS, L, S, stream())
    assert Lb.load().ldm_attention_folded(*args) != 0
    with pytest.raises(Lb.LDMError, match="no instance"):
        Lb.call("ldm_attention_folded", *args)
    out.untouched()


# ---- d. probabilities only -----------------------------------------------------------------------------
@pytest.mark.parametrize("L,S", [(1, 1), (6, 16), (16, 6), (10, 10), (16, 16)])
def test_folded_probs(cuda, L, S):
    from ldm_amd import _lib as Lb
    E = 512
    c = fold_case(E, L, S)
    dv, kf, bf = raw_fold_keys(cuda, c)
    p = Guarded((B, HEADS, L, S), cuda)
    Lb.call("ldm_attention_folded_probs", dv["z"].data_ptr(), kf.data_ptr(), bf.data_ptr(), p.ptr(), B, E, HEADS, L, S,
            stream())
    got = p.written()
    check(got, c["p"], TOL_FOLD, "p", f"probs L={L} S={S}")
    assert np.abs(npy(got).sum(-1) - 1.0).max() < 1e-6


# ---- e. softmax range ----------------------------------------------------------------------------------
RANGE_SHAPES = [(256, 40, 64), (512, 12, 16)]
RANGE = [(E, L, S, v) for (E, L, S) in RANGE_SHAPES for v in ("wide", "onehot")]


@functools.lru_cache(maxsize=None)
def range_case(E, L, S, variant):
    """wide: q scaled so that the float64 logits span +-60.  onehot: q[., l] of head h is a multiple of key
    hot[b, h, l], large enough that this key's logit beats every other by more than 100.  The folded form gets the same
    queries through an orthogonal Wq: z = Wq^T (q - bq), so that Wq z + bq gives them back to fp32 rounding."""
    d = E // HEADS
    g = torch.Generator().manual_seed(31 * E + 64 * L + S + (1 if variant == "wide" else 2))
    q = torch.randn(B, E, L, generator=g)
    kv = torch.randn(B, 2 * E, S, generator=g)
    dout = torch.randn(B, E, L, generator=g)
    wq = torch.linalg.qr(torch.randn(E, E, generator=g).double())[0]
    bq = torch.randn(E, generator=g) * 0.1
    b_, h_, l_ = torch.meshgrid(torch.arange(B), torch.arange(HEADS), torch.arange(L), indexing="ij")
    hot = (5 * l_ + 3 * h_ + b_) % S                                              # [B,h,L]
    if variant == "wide":
        q = (q.double() * (60.0 / logits64(q, kv).abs().max())).float()
    else:
        k = kv[:, :E].reshape(B, HEADS, d, S)
        qh = torch.gather(k, 3, hot[:, :, None, :].expand(B, HEADS, d, L))       # [B,h,d,L] = K[b,h,:,hot]
        lg = logits64(qh.reshape(B, E, L), kv)
        gap = torch.gather(lg, 3, hot[..., None])[..., 0] - lg.scatter(3, hot[..., None], -math.inf).max(-1).values
        q = (qh.reshape(B, E, L).double() * (130.0 / gap.min())).float()
    wq = wq.float().contiguous()   # (qr returns Q column-major)
    z =torch.einsum("oe,bol->ble", wq.double(), q.double() - bq.double()[None, :, None]).float()
    c = {"q": q, "kv": kv, "dout": dout, "z": z, "wq": wq, "bq": bq, "hot": hot}
    c["y"], c["dq"], c["dkv"] = grads(q.double(), kv.double(), dout.double())
    c["yf"] = folded(z.double(), kv.double(), wq.double(), bq.double())
    # the inputs are what the variant promises, for the direct and for the folded queries
    qf = (torch.einsum("oe,ble->blo", wq.double(), z.double()) + bq.double()).transpose(1, 2)
    for lg in (logits64(q, kv), logits64(qf, kv)):
        if variant == "wide":
            assert 55.0 < lg.abs().max() < 65.0
        else:
            top = torch.gather(lg, 3, hot[..., None])[..., 0]
            assert (top - lg.scatter(3, hot[..., None], -math.inf).max(-1).values).min() > 100.0
    v = kv[:, E:].reshape(B, HEADS, d, S)
    c["vhot"] = torch.gather(v, 3, hot[:, :, None, :].expand(B, HEADS, d, L)).reshape(B, E, L)   # V[b,h,:,hot] per query
    return c


# (rel_err, worst row) of fp32 CPU torch of the same formulas against float64 on range_case's inputs; the kernels sum
# the same fp32 products in another order and are allowed 4x.  yf: the folded form's output.
RANGE_REF = {
    (256, 40, 64, "wide"): {"y": (1.6e-06, 4.1e-06), "yf": (4.0e-06, 8.5e-06), "dq": (2.1e-06, 1.1e+00),
                            "dK": (2.4e-06, 4.2e-03), "dV": (1.3e-06, 1.7e-05)},
    (512, 12, 16, "wide"): {"y": (3.7e-06, 8.1e-06), "yf": (3.9e-06, 9.0e-06), "dq": (4.1e-06, 2.5e+00),
                            "dK": (4.1e-06, 3.4e-02), "dV": (1.9e-06, 1.6e-05)},
    # one-hot rows: exp of anything below -104 is 0 in fp32 and 1e-57 in float64, so P is exactly one-hot in both, y is
    # exactly a V column and (every key here is the hot key of at most one query) dV exactly a dO column: error 0.
    # dV's figures are the float64 columns of keys that no query picked (1e-57, 0 in fp32; per row against the 1e-30
    # floor of row_err)
    (256, 40, 64, "onehot"): {"y": (0.0, 0.0), "yf": (0.0, 0.0), "dV": (2.1e-57, 8.7e-27)},
    (512, 12, 16, "onehot"): {"y": (0.0, 0.0), "yf": (0.0, 0.0), "dV": (5.5e-63, 2.0e-32)},
}


def range_tols(E, L, S, variant, names):
    ref = RANGE_REF[(E, L, S, variant)]
    return {n: 4 * ref[n][0] for n in names}, {n: 4 * ref[n][1] for n in names}


def hot_columns(y, c, what):
    """one-hot rows are that key's V column (1e-6 relative, over the tensor and per row)"""
    check(y, c["vhot"], 1e-6, "cm", what + " against V[hot]")


@pytest.mark.parametrize("E,L,S,variant", RANGE)
def test_range_forward(cuda, E, L, S, variant):
    """ldm_attention_core with logits spanning +-60 (wide) and with one key per row ahead by more than 100 (onehot):
    the -inf max seed, the masked expf and the padded columns' zeros under range.  Bound: 4x the error of fp32 CPU
    torch against float64 on the same inputs.  Measured reference error (rel_err, worst row) / resulting bound:
    E 256 (40, 64) wide 1.6e-6, 4.1e-6 / 6.4e-6, 1.6e-5; E 512 (12, 16) wide 3.7e-6, 8.1e-6 / 1.5e-5, 3.2e-5; onehot
    0, 0 / 0, 0 (both exactly the hot key's V column, see RANGE_REF)."""
    c = range_case(E, L, S, variant)
    tol, row = range_tols(E, L, S, variant, ["y"])
    out = raw_forward(cuda, c["q"], c["kv"])
    check(out, c["y"], tol["y"], "cm", f"range forward E={E} L={L} S={S} {variant}", row["y"])
    if variant == "onehot":
        hot_columns(out, c, "range forward")


@pytest.mark.parametrize("E,L,S,variant", RANGE)
def test_range_folded(cuda, E, L, S, variant):
    """ldm_attention_fold_keys + ldm_attention_folded on the same queries (z = Wq^T (q - bq), Wq orthogonal).  Measured
    reference error (rel_err, worst row) / resulting bound (4x): E 256 (40, 64) wide 4.0e-6, 8.5e-6 / 1.6e-5, 3.4e-5;
    E 512 (12, 16) wide 3.9e-6, 9.0e-6 / 1.6e-5, 3.6e-5; onehot 0, 0 / 0, 0."""
    c = range_case(E, L, S, variant)
    tol, row = range_tols(E, L, S, variant, ["yf"])
    out = raw_folded(cuda, c)
    check(out, c["yf"], tol["yf"], "tm", f"range folded E={E} L={L} S={S} {variant}", row["yf"])
    if variant == "onehot":
        hot_columns(out.transpose(1, 2), c, "range folded")


@pytest.mark.parametrize("E,L,S,variant", RANGE)
def test_range_backward(cuda, E, L, S, variant):
    """functional.attention_core forward + backward (both shapes take the scalar form).  Measured reference error
    (rel_err, worst row) of y, dq, dK, dV / resulting bound (4x), wide:
      E 256 (40, 64): y 1.6e-6, 4.1e-6; dq 2.1e-6, 1.1; dK 2.4e-6, 4.2e-3; dV 1.3e-6, 1.7e-5
                      / y 6.4e-6, 1.6e-5; dq 8.4e-6, 4.4; dK 9.6e-6, 1.7e-2; dV 5.2e-6, 6.8e-5
      E 512 (12, 16): y 3.7e-6, 8.1e-6; dq 4.1e-6, 2.5; dK 4.1e-6, 3.4e-2; dV 1.9e-6, 1.6e-5
                      / y 1.5e-5, 3.2e-5; dq 1.6e-5, 10; dK 1.6e-5, 0.14; dV 7.6e-6, 6.4e-5
    (a saturated query's dq row and an unattended key's dK row are ~1e-20 of the tensor's largest: fp32 itself is off
    by more than the row there, so dq's per-row bound says nothing and only the tensor-wide one binds).
    onehot: y 0 / 0 and dV 2.1e-57, 8.7e-27 / 8.4e-57, 3.5e-26 (E 256), 5.5e-63, 2.0e-32 / 2.2e-62, 8.0e-32 (E 512):
    exact up to float64's own 1e-57 columns, see RANGE_REF.  dq and dK are compared with nothing: every off-key probability is
    below exp(-100) = 4e-44, so the float64 gradients are below 1e-50 of dV's, and |dq|, |dK| < 1e-30 is asserted."""
    c = range_case(E, L, S, variant)
    names = ["y", "dq", "dK", "dV"] if variant == "wide" else ["y", "dV"]
    tol, row = range_tols(E, L, S, variant, names)
    y, dq, dkv = autograd_backward(cuda, c)
    assert all(bool(torch.isfinite(t).all()) for t in (y, dq, dkv))
    what = f"range backward E={E} L={L} S={S} {variant}"
    if variant == "wide":
        check_grads(y, dq, dkv, c, E, what, tol, row)
    else:
        check(y, c["y"], tol["y"], "cm", what + " y", row["y"])
        check(dkv[:, E:], c["dkv"][:, E:], tol["dV"], "cm", what + " dV", row["dV"])
        hot_columns(y, c, what)
        assert float(c["dq"].abs().max()) < 1e-30 and float(c["dkv"][:, :E].abs().max()) < 1e-30
        assert float(dq.abs().max()) < 1e-30 and float(dkv[:, :E].abs().max()) < 1e-30
