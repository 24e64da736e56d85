"""CA1's folded keys in MFMA fragment order for the reverse loop's probabilities kernel (csrc/bfold.hip).  The packed
form is a permutation of the plain [B, 4, 16, 512] layout and its kernel runs the plain kernel's sums in the plain
kernel's order, so everything here is exact (torch.equal): the packed keys un-permuted on the host with the index
formula of include/ldm_capi.h against the plain ones, ldm_ca1_probs_packed against ldm_ca1_probs, the bottleneck fed
by either, and a short sampling loop with LDM_BFOLD_PACKED=0 against the default.  The kernels are fixed-shape (2 x 8
plane, E = 512, 4 heads, 16 keys); B = 1, 3 (odd: a wrong sample stride) and 8 (the fold's upper limit).  The same
order for the bottleneck's folded values U was built and measured no faster (profiles/r10), so U has no packed form
and none is tested."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 8)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _operands(B, seed):
    g = torch.Generator().manual_seed(seed)
    z4 = torch.rand(B, 16, 512, generator=g)                          # token-major (NHWC on the 2 x 8 plane)
    kf = torch.randn(B, 4, 16, 512, generator=g) * 0.05
    bf = torch.randn(B, 4, 16, generator=g) * 0.1
    kv = torch.randn(B, 1024, 16, generator=g)
    wf = torch.randn(512, 512, 3, 3, generator=g) / np.sqrt(4608.0)
    pb = torch.randn(16, 512, generator=g) * 0.1                      # position-major bias [l][co]
    return z4, kf, bf, kv, wf, pb


def _keys_packed_index(B):
    """Float index in the packed keys of every element [b][h][s][e] of the plain ones (ldm_capi.h)."""
    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(4).view(1, 4, 1, 1)
    s = torch.arange(16).view(1, 1, 16, 1)
    e = torch.arange(512).view(1, 1, 1, 512)
    return ((((((b * 4 + h) * 32 + e // 16) * 4 + (e % 16) // 4) * 16 + s) * 4 + e % 4)).reshape(-1)


def test_index_formula_is_a_permutation():
    for B in (1, 3):
        idx, n = _keys_packed_index(B), B * 4 * 16 * 512
        assert idx.numel() == n and torch.equal(torch.sort(idx).values, torch.arange(n))


@pytest.mark.parametrize("B", BATCHES)
def test_packed_keys_and_probs(cuda, B):
    from ldm_amd import _lib as L
    z4, kf, bf, kv, wf, pb = (t.to(cuda).contiguous() for t in _operands(B, 600 + B))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    kp = torch.full((B * 4 * 16 * 512,), float("nan"), device=cuda)
    p = torch.empty(B, 4, 16, 16, device=cuda)
    pp = torch.full((B, 4, 16, 16), float("nan"), device=cuda)
    L.call("ldm_ca1_pack_keys", _ptr(kf), _ptr(kp), B, st)
    L.call("ldm_ca1_probs", _ptr(z4), _ptr(kf), _ptr(bf), _ptr(p), B, st)
    L.call("ldm_ca1_probs_packed", _ptr(z4), _ptr(kp), _ptr(bf), _ptr(pp), B, st)
    torch.cuda.synchronize()
    assert torch.equal(kp[_keys_packed_index(B).to(cuda)].view(B, 4, 16, 512), kf)
    assert torch.equal(pp, p)
    assert torch.allclose(p.sum(-1), torch.ones(B, 4, 16, device=cuda), atol=1e-5)
    # the bottleneck on either P (what the loop's next launch reads)
    u = torch.empty(B, 512, 576, device=cuda)
    y, yp = torch.empty(B, 16, 512, device=cuda), torch.empty(B, 16, 512, device=cuda)
    L.call("ldm_bneck_fold_values", _ptr(wf), _ptr(kv), _ptr(u), B, st)
    L.call("ldm_bneck_pv", _ptr(u), _ptr(p), _ptr(pb), _ptr(y), B, 0, st)
    L.call("ldm_bneck_pv", _ptr(u), _ptr(pp), _ptr(pb), _ptr(yp), B, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(yp, y) and float(y.abs().max()) > 0.0


def child(out_path, want_mask):
    """Runs in the child process, the setting already in its environment: a 5-step loop at B = 3 on the canonical latent."""
    import models.model as M
    from ldm_amd import _lib as L
    lib = L.load()
    assert lib.ldm_bfold_packed_form() == want_mask, lib.ldm_bfold_packed_form()
    assert lib.ldm_bneck_fold_supported(3, 16, 64) == 1 and lib.ldm_ca1_probs_form() == 1
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(dev)
    g = torch.Generator().manual_seed(11)
    B, H, W = 3, 16, 64
    z = torch.randn(B, 32, H, W, generator=g).to(dev)
    emb = {"s5": torch.rand(B, 256, H // 4, W // 4, generator=g).to(dev),
           "s6": torch.rand(B, 512, H // 8, W // 8, generator=g).to(dev)}
    times = torch.tensor([180, 150, 120, 90, 60, 30])
    with torch.no_grad():
        x, logs = ldm._reverse(z, emb, times, 0.0)
    torch.cuda.synchronize()
    assert len(logs["pred_x0"]) == 5 and bool(torch.isfinite(x).all())
    torch.save({"x": x.cpu(), "pred_x0": torch.stack(logs["pred_x0"]).cpu(),
                "noise_pred": torch.stack(logs["noise_pred"]).cpu()}, out_path)


def test_loop_packed_equals_plain(cuda):
    here = os.path.dirname(os.path.abspath(__file__))
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, setting, mask in (("plain", "0", 0), ("packed", None, 1)):
            out = os.path.join(tmp, name + ".pt")
            code = ("import sys; sys.path.insert(0, %r); import conftest, test_gpu_bfold_packed as t; t.child(%r, %d)"
                    % (here, out, mask))
            env = {k: v for k, v in os.environ.items() if k not in ("LDM_BFOLD_PACKED", "LDM_BNECK_FOLD", "LDM_CA1P_FORM")}
            if setting is not None:
                env["LDM_BFOLD_PACKED"] = setting
            r = subprocess.run([sys.executable, "-c", code], env=env, cwd=here, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            got[name] = torch.load(out)
    for k in ("x", "pred_x0", "noise_pred"):
        assert torch.equal(got["packed"][k], got["plain"][k]), k
