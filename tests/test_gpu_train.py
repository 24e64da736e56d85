"""GPU parity of the TRAIN path (LDMTrainer.train_step, reference train.py:163-208) on the HIP kernels.

Layer backward kernels are checked against float64 torch-CPU autograd of the same op (plain PyTorch
reference, §How-to-work); the whole train step against golden gradients / Adam updates captured from the
REFERENCE (tests/golden/make_goldens.py section 7).  Tolerance: max|g - g_ref| <= 1e-4 * max|g_ref|
(north_star "within 1e-4 rel-fp32"); the optimiser update 1e-5 (elementwise, no reduction).
"""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

import recipe
from conftest import ROOT, adam_step_err, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().double().cpu().numpy()


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.uniform(lo, hi, shape).astype(np.float32)


# ---- conv / convT backward with fused epilogues ----------------------------------------------------
# (B, Cin, H, W, Cout, k, stride, pad, out_pad, transposed, act, bcast, skip)
CONV_CASES = {
    "unet_enc1_k3s1": (2, 32, 16, 16, 64, 3, 1, 1, 0, False, "relu", False, False),
    "unet_enc2_k3s2_temb": (2, 64, 16, 16, 128, 3, 2, 1, 0, False, "relu", True, False),
    "unet_bottleneck_k3s1": (2, 512, 2, 2, 512, 3, 1, 1, 0, False, "relu", False, False),
    "unet_dec4_convT_skip": (2, 512, 2, 2, 256, 3, 2, 1, 1, True, "relu", False, True),
    "unet_dec2_convT_skip": (2, 128, 8, 8, 64, 3, 2, 1, 1, True, "relu", False, True),
    "unet_dec1_k3s1_linear": (2, 64, 16, 16, 32, 3, 1, 1, 0, False, "none", False, False),
    "proj_1x1": (2, 256, 4, 4, 512, 1, 1, 0, 0, False, "none", False, False),
    "style_enc1_cin1": (2, 1, 32, 32, 64, 3, 2, 1, 0, False, "relu", False, False),
    "vae_dec_convT_k4": (2, 32, 4, 4, 128, 4, 2, 1, 0, True, "none", False, False),
    "vae_dec_out_tanh_half": (2, 64, 16, 16, 1, 4, 2, 1, 0, True, "tanh_half", False, False),
    "batch3_nonsquare_tanh": (3, 8, 6, 10, 16, 3, 2, 1, 0, False, "tanh", False, False),
    # Cin = 1 with Wout % 4 != 0: the one-output-per-lane kernel (the 4-column kernel needs Wout % 4 == 0)
    "cin1_k3s2_ragged_cols": (2, 1, 18, 22, 16, 3, 2, 1, 0, False, "relu", False, False),
    # the decoder output layer's shape class at a wider, non-square plane (4-column convT kernel, W4 = 10)
    "vae_dec_out_wide": (2, 64, 8, 40, 1, 4, 2, 1, 0, True, "tanh_half", False, False),
}


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv_backward(cuda, case):
    from ldm_amd import functional as HF
    B, Cin, H, W, Cout, k, s, p, op, tr, act, has_bc, has_sk = CONV_CASES[case]
    seed = zlib.crc32(case.encode()) % 1000
    x = _rand((B, Cin, H, W), seed)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w = _rand(wshape, seed + 1, -0.2, 0.2)
    b = _rand((Cout,), seed + 2, -0.1, 0.1)
    xt = torch.from_numpy(x).double().requires_grad_()
    wt = torch.from_numpy(w).double().requires_grad_()
    bt = torch.from_numpy(b).double().requires_grad_()
    if tr:
        v = tF.conv_transpose2d(xt, wt, bt, stride=s, padding=p, output_padding=op)
    else:
        v = tF.conv2d(xt, wt, bt, stride=s, padding=p)
    a = {"none": lambda u: u, "relu": torch.relu, "tanh": torch.tanh,
         "tanh_half": lambda u: (torch.tanh(u) + 1) / 2}[act](v)
    extra_cpu, extra_gpu = [], []
    if has_bc:
        bc = _rand((B, Cout), seed + 3)
        bct = torch.from_numpy(bc).double().requires_grad_()
        a = a + bct[:, :, None, None]
        extra_cpu.append(bct)
        extra_gpu.append(T(bc, cuda).requires_grad_())
    if has_sk:
        sk = _rand(tuple(a.shape), seed + 4)
        skt = torch.from_numpy(sk).double().requires_grad_()
        a = a + skt
        extra_cpu.append(skt)
        extra_gpu.append(T(sk, cuda).requires_grad_())
    R = _rand(tuple(a.shape), seed + 5)
    (a * torch.from_numpy(R).double()).sum().backward()

    xg, wg, bg = (T(v_, cuda).requires_grad_() for v_ in (x, w, b))
    y = HF.conv(xg, wg, bg, stride=s, padding=p, transposed=tr, output_padding=op, act=act,
                bcast=extra_gpu[0] if has_bc else None, skip=extra_gpu[-1] if has_sk else None)
    assert rel_err(npy(y), a.detach().numpy()) < TOL
    (y * T(R, cuda)).sum().backward()
    assert rel_err(npy(xg.grad), xt.grad.numpy()) < TOL, "dx"
    assert rel_err(npy(wg.grad), wt.grad.numpy()) < TOL, "dw"
    assert rel_err(npy(bg.grad), bt.grad.numpy()) < TOL, "db"
    for gt, ct in zip(extra_gpu, extra_cpu):
        assert rel_err(npy(gt.grad), ct.grad.numpy()) < TOL, "dbcast/dskip"


def test_ragged_stride2_backward_raises(cuda):
    """Odd spatial sizes: the stride-2 data gradient needs a ragged transposed conv, not supported
    (the model's shapes are all even: 128x512 -> 16x64 -> 2x8); it must raise, not return garbage."""
    from ldm_amd import functional as HF
    x = T(_rand((1, 8, 7, 9), 5), cuda).requires_grad_()
    w = T(_rand((16, 8, 3, 3), 6), cuda).requires_grad_()
    y = HF.conv(x, w, None, stride=2, padding=1)
    with pytest.raises(RuntimeError):
        y.sum().backward()


def test_linear_and_gelu_backward(cuda):
    from ldm_amd import functional as HF
    x = _rand((3, 128), 11)
    w1, b1 = _rand((128, 128), 12, -0.1, 0.1), _rand((128,), 13, -0.1, 0.1)
    xt, w1t, b1t = (torch.from_numpy(v).double().requires_grad_() for v in (x, w1, b1))
    ref = tF.gelu(tF.linear(xt, w1t, b1t))
    R = _rand((3, 128), 14)
    (ref * torch.from_numpy(R).double()).sum().backward()
    xg, w1g, b1g = (T(v, cuda).requires_grad_() for v in (x, w1, b1))
    y = HF.activation(HF.linear(xg, w1g, b1g), "gelu")
    (y * T(R, cuda)).sum().backward()
    assert rel_err(npy(y), ref.detach().numpy()) < TOL
    for g, r in ((xg, xt), (w1g, w1t), (b1g, b1t)):
        assert rel_err(npy(g.grad), r.grad.numpy()) < TOL


@pytest.mark.parametrize("shape", [(4, 64, 8, 8), (3, 8, 36, 36), (5, 4, 30, 30), (3, 6, 7, 9), (32, 16, 16, 64)])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_batchnorm_train_backward(cuda, act, shape):
    """Train-mode BN forward / backward against fp64 autograd; the shapes force several slices per
    channel (P > 1), slices crossing plane boundaries, the three access widths (8 elements: HW % 8 == 0,
    float4: HW = 900, scalar: HW = 63) and the B=32 form."""
    from ldm_amd import nn as hnn
    C = shape[1]
    x = _rand(shape, 21, -2, 2)
    bn_ref = torch.nn.BatchNorm2d(C).double()
    bn = hnn.BatchNorm2d(C).to(cuda)
    with torch.no_grad():
        g = torch.from_numpy(_rand((C,), 22, 0.5, 1.5))
        b = torch.from_numpy(_rand((C,), 23, -0.1, 0.1))
        bn_ref.weight.copy_(g.double())
        bn_ref.bias.copy_(b.double())
        bn.weight.copy_(g.to(cuda))
        bn.bias.copy_(b.to(cuda))
    xt = torch.from_numpy(x).double().requires_grad_()
    ref = bn_ref(xt)
    if act == "relu":
        ref = torch.relu(ref)
    R = _rand(shape, 24)
    (ref * torch.from_numpy(R).double()).sum().backward()
    xg = T(x, cuda).requires_grad_()
    y = bn(xg, act=act)
    (y * T(R, cuda)).sum().backward()
    assert rel_err(npy(y), ref.detach().numpy()) < TOL
    assert rel_err(npy(xg.grad), xt.grad.numpy()) < TOL
    assert rel_err(npy(bn.weight.grad), bn_ref.weight.grad.numpy()) < TOL
    assert rel_err(npy(bn.bias.grad), bn_ref.bias.grad.numpy()) < TOL
    assert rel_err(npy(bn.running_var), bn_ref.running_var.numpy()) < TOL


@pytest.mark.parametrize("E,L", [(256, 64), (512, 16), (256, 4), (512, 36)])
def test_attention_backward(cuda, E, L):
    """CA2 (E=256, d=64, L=S=64) and CA1 (E=512, d=128, L=S=16) core backward on the MFMA form; L=S=4
    (a 16x16 latent's CA1) and 36 on the scalar form (dims not multiples of 16).  These are the model's own
    L = S planes only: L != S, the ragged side of every padded instance, head dims 24 / 32, the scalar form's
    LDS limit (d = 128 holds L = S <= 46) and the shapes beyond it that go to the KV-tiled backward are swept
    in test_gpu_attention_small.py."""
    from ldm_amd import functional as HF
    heads, B = 4, 2
    d = E // heads
    q = _rand((B, E, L), 31)
    kv = _rand((B, 2 * E, L), 32)
    qt = torch.from_numpy(q).double().requires_grad_()
    kvt = torch.from_numpy(kv).double().requires_grad_()
    qh = qt.view(B, heads, d, L)
    kh = kvt[:, :E].reshape(B, heads, d, L)
    vh = kvt[:, E:].reshape(B, heads, d, L)
    P = torch.softmax(torch.einsum("bhcl,bhcs->bhls", qh * (1.0 / d) ** 0.5, kh), -1)
    ref = torch.einsum("bhls,bhcs->bhcl", P, vh).reshape(B, E, L)
    R = _rand((B, E, L), 33)
    (ref * torch.from_numpy(R).double()).sum().backward()
    qg, kvg = T(q, cuda).requires_grad_(), T(kv, cuda).requires_grad_()
    y = HF.attention_core(qg, kvg, heads)
    (y * T(R, cuda)).sum().backward()
    assert rel_err(npy(y), ref.detach().numpy()) < TOL
    assert rel_err(npy(qg.grad), qt.grad.numpy()) < TOL
    assert rel_err(npy(kvg.grad), kvt.grad.numpy()) < TOL


# ---- optimiser ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "adamw", "adam_wd"])
def test_adam_matches_torch(cuda, kind):
    from ldm_amd import optim as hoptim
    shapes = [(64, 32, 3, 3), (64,), (300001,), (7, 5)]
    ps_ref = [torch.nn.Parameter(torch.from_numpy(_rand(s, 40 + i))) for i, s in enumerate(shapes)]
    ps = [torch.nn.Parameter(p.detach().clone().to(cuda)) for p in ps_ref]
    kw = dict(lr=5e-4)
    if kind == "adam":
        ref, mine = torch.optim.Adam(ps_ref, **kw), hoptim.Adam(ps, **kw)
    elif kind == "adam_wd":
        ref, mine = torch.optim.Adam(ps_ref, weight_decay=0.01, **kw), hoptim.Adam(ps, weight_decay=0.01, **kw)
    else:
        ref, mine = torch.optim.AdamW(ps_ref, **kw), hoptim.AdamW(ps, **kw)
    for step in range(3):
        for i, (a, b) in enumerate(zip(ps_ref, ps)):
            g = torch.from_numpy(_rand(a.shape, 100 * step + i))
            a.grad = g.clone()
            b.grad = g.to(cuda)
        ref.step()
        mine.step()
    for a, b in zip(ps_ref, ps):
        assert rel_err(npy(b), a.detach().double().numpy()) < 1e-6
    st = mine.state_dict()
    assert st["state"][0]["step"].item() == 3 and set(st["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # torch's LR scheduler drives it unchanged
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(mine, factor=0.5, patience=0)
    sch.step(1.0)
    sch.step(2.0)
    assert mine.param_groups[0]["lr"] == pytest.approx(2.5e-4)


def test_grad_scaler_skip_backoff_growth(cuda):
    from ldm_amd import optim as hoptim
    p = torch.nn.Parameter(torch.ones(1000, device=cuda))
    opt = hoptim.Adam([p], lr=0.1)
    sc = hoptim.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    # inf gradient: step skipped, scale backs off
    p.grad = torch.full((1000,), float("inf"), device=cuda)
    sc.step(opt)
    sc.update()
    assert sc.get_scale() == 512.0 and torch.all(p.detach() == 1.0)
    assert len(opt.state) == 0
    # clean steps: unscaled grad applied, growth after 2
    for _ in range(2):
        p.grad = torch.full((1000,), 512.0 * 0.5, device=cuda) * (sc.get_scale() / 512.0)
        sc.step(opt)
        sc.update()
    assert sc.get_scale() == 1024.0
    assert float(opt.state[p]["step"]) == 2.0
    assert torch.all(p.detach() < 1.0)


# ---- whole train step vs the reference ----------------------------------------------------------------
GRAD_KEYS = ("unet.time_mlp.1.weight", "unet.dec1.weight", "unet.dec1.bias", "unet.enc1.weight",
             "unet.cross_attention1.multihead_attn.in_proj_weight", "unet.bottleneck.bias",
             "decoder.decoder.6.weight", "decoder.decoder.1.weight", "style_encoder.enc6.bias",
             "style_encoder.enc1.weight")


def test_train_step_matches_reference(goldens, cuda):
    """train_step restated in make_goldens.py (fp32, no LPIPS/VGGish): encoder frozen, model.train(),
    loss = MSE(recon, x) + 0.01 KL(z0) + MSE(eps_pred, eps); Adam(lr=5e-4) step."""
    import models.loss as Lm
    import models.model as M
    from ldm_amd import optim as hoptim
    ldm = M.LDM(32, pretrained_path="")
    recipe.fill_module(ldm, seed=700)
    ldm = ldm.to(cuda)
    ldm.train()
    for p in ldm.encoder.parameters():
        p.requires_grad_(False)
    opt = hoptim.Adam([p for p in ldm.parameters() if p.requires_grad], lr=5e-4)
    content = T(recipe.uniform01((2, 1, 128, 128), 710), cuda)
    style = T(recipe.uniform01((2, 1, 128, 128), 711), cuda)
    t = T(goldens["fwd_eval_t"], cuda)
    noise = T(goldens["train_noise"], cuda)
    opt.zero_grad()
    out = ldm(content, style, t, noise=noise)
    # compression_loss with config 'lpips' and no LPIPS backend = MSE + 0.01 KL (as the golden step)
    total = Lm.compression_loss(content, out["reconstructed"], out["z_0"], None) + \
        Lm.diffusion_loss(out["noise_pred"], out["noise"])
    total.backward()
    assert rel_err(npy(out["reconstructed"]), goldens["train_recon"]) < TOL
    assert rel_err(npy(total), goldens["train_total"]) < TOL
    named = dict(ldm.named_parameters())
    for k in GRAD_KEYS:
        g = named[k].grad
        g = g[:256] if g.dim() == 2 and g.shape[0] > 256 else g
        assert rel_err(npy(g), goldens["grad_" + k]) < TOL, k
    opt.step()
    for k in ("unet.dec1.weight", "decoder.decoder.6.weight", "style_encoder.enc6.bias"):
        assert rel_err(npy(named[k]), goldens["adam1_" + k]) < 1e-5, k
    assert rel_err(npy(ldm.encoder.encoder[1].running_mean), goldens["train_enc_rm0"]) < TOL
    assert rel_err(npy(ldm.decoder.decoder[4].running_var), goldens["train_dec_rv1"]) < TOL


class _ZeroFeat(torch.nn.Module):
    """Perceptual feature net stand-in: 0 (LPIPS/VGGish are out of scope offline; the golden train step
    omits them too)."""

    def forward(self, a, b):
        return torch.zeros((), device=a.device)


def test_second_step_uses_updated_weights(cuda):
    """After an optimizer step the next forward must see the new weights: the fused Adam writes them through
    raw pointers, so it has to move their versions or the packed-weight caches keep serving the old ones.
    Step 2 of one trainer == step 1 of a fresh model loaded with the trainer's state after step 1."""
    import models.model as M
    import models.train as TR
    content = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), 850)).to(cuda)
    style = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), 851)).to(cuda)
    t = torch.tensor([10, 150], device=cuda)
    noise = torch.from_numpy(recipe.normal((2, 32, 16, 16), 852)).to(cuda)
    a = M.LDM(32, pretrained_path="")
    recipe.fill_module(a, seed=700)
    a.feature_loss_net = _ZeroFeat()
    a = a.to(cuda).train()
    ta = TR.LDMTrainer(a, [], cuda, lr=1e-3)
    for tr in (ta,):
        tr.autocast_enabled = False
    ta.train_step(content, style, t=t, noise=noise)
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    l2 = ta.train_step(content, style, t=t, noise=noise)
    b = M.LDM(32, pretrained_path="")
    b.feature_loss_net = _ZeroFeat()
    b.load_state_dict(sd)
    b = b.to(cuda).train()
    tb = TR.LDMTrainer(b, [], cuda, lr=1e-3)
    tb.autocast_enabled = False
    l1b = tb.train_step(content, style, t=t, noise=noise)
    for k in ("total_loss", "denoisinsg_loss", "compression_loss"):
        assert abs(l2[k] - l1b[k]) <= 1e-5 * abs(l1b[k]), (k, l2[k], l1b[k])


@pytest.mark.parametrize("autocast,mode", [(False, "thread_local"), (True, "thread_local"), (True, "global")])
def test_graphed_train_step_equals_eager(cuda, autocast, mode, monkeypatch):
    """LDMTrainer.graph_step: 2 eager warm-up steps, then the step captured into a hipGraph and replayed.
    With injected t / noise the eight steps' losses and the final parameters and BN buffers equal an eager
    trainer's bitwise (same kernels; the capturable Adam forms its scalars from the device step count
    exactly as the host form does); under autocast too; a learning-rate change after step 5 re-captures.
    mode "global": the capture in the global capture mode, in which an unsafe runtime call from ANY thread --
    the backward runs on autograd's device thread -- fails the capture instead of running at capture time and
    missing from the replays (the product captures in the thread-local mode, ldm_amd/graphs.py)."""
    import models.model as M
    import models.train as TR
    from ldm_amd import graphs as hgraphs
    monkeypatch.setenv("LDM_AMD_CAPTURE_MODE", mode)
    assert hgraphs.capture_mode() == mode
    content = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), 860)).to(cuda)
    style = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), 861)).to(cuda)
    t = torch.tensor([10, 150], device=cuda)
    noise = torch.from_numpy(recipe.normal((2, 32, 16, 16), 862)).to(cuda)
    res = []
    for graph in (False, True):
        m = M.LDM(32, pretrained_path="")
        recipe.fill_module(m, seed=700)
        m.feature_loss_net = _ZeroFeat()
        m = m.to(cuda).train()
        tr = TR.LDMTrainer(m, [], cuda, lr=1e-3)
        tr.autocast_enabled = autocast
        tr.graph_step = graph
        losses = [tr.train_step(content, style, t=t, noise=noise) for _ in range(5)]
        assert (tr._graph is not None) == graph
        # a learning-rate change (ReduceLROnPlateau between epochs) must reach the graphed step too
        tr.optimizer.param_groups[0]["lr"] *= 0.5
        losses += [tr.train_step(content, style, t=t, noise=noise) for _ in range(3)]
        res.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    (le, sde), (lg, sdg) = res
    for a, b in zip(le, lg):
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    for k in sde:
        assert torch.equal(sde[k], sdg[k]), k


def test_graphed_train_step_inf_skips_like_eager(cuda):
    """GradScaler's inf/nan skip inside the graph: step 4 of 7 gets a non-finite noise target, so its
    gradients are non-finite; Adam must skip it (capturable form: on the device, step count held) and the
    scale back off once, exactly as the eager step with its host-side found_inf read.  Bitwise equal."""
    import models.model as M
    import models.train as TR
    content = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), 870)).to(cuda)
    style = torch.from_numpy(recipe.uniform01((2, 1, 128, 128), 871)).to(cuda)
    t = torch.tensor([30, 170], device=cuda)
    noise = torch.from_numpy(recipe.normal((2, 32, 16, 16), 872)).to(cuda)
    bad = noise.clone()
    bad[0, 0, 0, 0] = float("inf")
    seq = [noise, noise, noise, bad, noise, noise, noise]
    res = []
    for graph in (False, True):
        m = M.LDM(32, pretrained_path="")
        recipe.fill_module(m, seed=700)
        m.feature_loss_net = _ZeroFeat()
        m = m.to(cuda).train()
        tr = TR.LDMTrainer(m, [], cuda, lr=1e-3)
        tr.autocast_enabled = False
        tr.graph_step = graph
        losses = [tr.train_step(content, style, t=t, noise=nz) for nz in seq]
        assert (tr._graph is not None) == graph
        res.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, tr.scaler.get_scale()))
    (le, sde, se), (lg, sdg, sg) = res
    assert se == sg == 2.0 ** 15, (se, sg)
    assert not np.isfinite(le[3]["total_loss"]) and all(np.isfinite(le[i]["total_loss"]) for i in (4, 5, 6))
    for a, b in zip(le, lg):
        for k in a:
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])
    for k in sde:   # (the non-finite step also reaches the BN running statistics, as in torch)
        a, b = sde[k], sdg[k]
        same = (a == b) | (torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else a == b
        assert bool(same.all()), k


def test_graphed_train_step_draws_t_and_noise(cuda):
    """graph_step with t / noise drawn inside the graph: replays advance the RNG (losses differ step to
    step) and training proceeds (finite, decreasing over 8 steps)."""
    import models.model as M
    import models.train as TR
    torch.manual_seed(0)
    m = M.LDM(32, pretrained_path="")
    m.feature_loss_net = _ZeroFeat()
    m = m.to(cuda).train()
    tr = TR.LDMTrainer(m, [], cuda, lr=1e-3)
    tr.graph_step = True
    content = torch.rand(4, 1, 128, 128, device=cuda)
    style = torch.rand(4, 1, 128, 128, device=cuda)
    losses = [tr.train_step(content, style)["total_loss"] for _ in range(8)]
    assert tr._graph is not None and all(np.isfinite(losses))
    assert len(set(losses[2:])) == len(losses[2:])
    assert np.mean(losses[-3:]) < np.mean(losses[:3])


def test_trainer_step_runs_and_decreases_loss(cuda):
    """LDMTrainer.train_step end to end (GradScaler + Adam + autocast context) on random data."""
    import models.model as M
    import models.train as TR
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").to(cuda)
    ldm.feature_loss_net = _ZeroFeat()
    for p in ldm.encoder.parameters():
        p.requires_grad_(False)
    ldm.train()
    tr = TR.LDMTrainer(ldm, [], cuda, lr=1e-3)
    content = torch.rand(2, 1, 128, 128, device=cuda)
    style = torch.rand(2, 1, 128, 128, device=cuda)
    t = torch.tensor([10, 150], device=cuda)
    noise = torch.randn(2, 32, 16, 16, device=cuda)
    losses = [tr.train_step(content, style, t=t, noise=noise)["total_loss"] for _ in range(5)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


# ---- train_autoencoder ------------------------------------------------------------
def test_autoencoder_step_matches_reference(goldens2, cuda):
    """models.train.autoencoder_step (the inner iteration of train_autoencoder, reference train.py:69-82)
    on the HIP path: train-mode BN in encoder and decoder, gradients through the whole encoder, fused
    AdamW — against the reference's own step (tests/golden/make_goldens.py --r2, LPIPS term left out)."""
    import models.model as M
    import models.train as TR
    from conftest import AE_KEYS
    from ldm_amd import optim as hoptim
    enc, dec = M.SpectrogramEncoder(32), M.SpectrogramDecoder(32)
    recipe.fill_module(enc, seed=730)
    recipe.fill_module(dec, seed=731)
    enc, dec = enc.to(cuda), dec.to(cuda)
    enc.train()
    dec.train()
    opt = hoptim.AdamW(list(enc.parameters()) + list(dec.parameters()), lr=5e-4)
    spec = T(recipe.uniform01((2, 1, 128, 128), 732), cuda)
    named = dict([("encoder." + k, v) for k, v in enc.named_parameters()] +
                 [("decoder." + k, v) for k, v in dec.named_parameters()])
    w0 = {k: npy(v) for k, v in named.items()}
    loss = TR.autoencoder_step(enc, dec, opt, spec, None)
    assert rel_err(npy(loss), goldens2["ae_loss"]) < TOL
    # float64 restatement of the same step (oracle, fixture-pinned in test_oracle_golden.py).  The
    # reference's own fp32 encoder gradients sit up to 6e-4 (relative to max) from float64: the train-mode
    # BN backward subtracts the channel means of 32k-element sums.  So each gradient is held to
    # max(1e-4, 3 x the reference's own fp32 error) against float64, and the conv biases that feed a
    # train-mode BN (mathematically zero gradient) to 1e-4 of the largest weight gradient.
    from oracle import ldm_torch_cpu as TC
    sd64 = {k: torch.from_numpy(v).double().requires_grad_("running" not in k) for k, v in w0.items()}
    for mod, pre in ((enc, "encoder."), (dec, "decoder.")):
        rs = M.SpectrogramEncoder(32) if pre == "encoder." else M.SpectrogramDecoder(32)
        recipe.fill_module(rs, seed=730 if pre == "encoder." else 731)
        for k, v in rs.state_dict().items():
            if "running" in k:
                sd64[pre + k] = v.double()
    x64 = spec.double().cpu()
    lat = TC.encoder(sd64, x64, True, state={})
    rec = TC.decoder(sd64, lat, True, state={})
    (tF.mse_loss(rec, x64) + 0.01 * TC.kl_loss(lat)).backward()
    gmax = max(np.abs(sd64[k].grad.numpy()).max() for k in ("encoder.encoder.0.weight", "encoder.encoder.3.weight"))
    for k in AE_KEYS + ("encoder.encoder.0.bias", "encoder.encoder.3.bias"):
        g64 = sd64[k].grad.numpy()
        if k in ("encoder.encoder.0.bias", "encoder.encoder.3.bias", "encoder.encoder.6.bias"):
            assert np.abs(npy(named[k].grad)).max() <= 1e-4 * gmax, k
            continue
        tol = max(TOL, 3 * rel_err(goldens2["ae_grad_" + k], g64))
        assert rel_err(npy(named[k].grad), g64) < tol, (k, tol)
    # AdamW's first step moves every element by ~lr * sign(g): elements with gradients inside the fp32
    # noise may move the other way (conftest.adam_step_err); the pre-BN encoder bias has no signal at all
    adam_grads = {k: npy(named[k].grad) for k in AE_KEYS}
    for k in AE_KEYS:
        if k == "encoder.encoder.6.bias":
            continue
        assert adam_step_err(npy(named[k]), goldens2["ae_adamw1_" + k], goldens2["ae_grad_" + k], 5e-4,
                             rel=2e-3, grad=adam_grads[k]) < 1e-5, k
    # ... and, element by element including the below-noise ones, the update is exactly AdamW's first step
    # on OUR gradient (float64 restatement of torch.optim.AdamW: decoupled decay, bias-corrected moments):
    # a sign or bias-correction error anywhere fails here whatever the gradient noise
    grp = opt.param_groups[0]
    lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
    for k in AE_KEYS:
        g = adam_grads[k].astype(np.float64)
        p0 = w0[k].astype(np.float64)
        m_hat = ((1 - b1) * g) / (1 - b1)
        v_hat = ((1 - b2) * g * g) / (1 - b2)
        want = p0 * (1 - lr * wd) - lr * m_hat / (np.sqrt(v_hat) + eps)
        err = np.abs(npy(named[k]) - want).max()
        assert err <= 1e-6 * (np.abs(p0).max() + lr), (k, err)
    assert rel_err(npy(enc.encoder[4].running_mean), goldens2["ae_enc_rm4"]) < TOL
    assert rel_err(npy(dec.decoder[1].running_var), goldens2["ae_dec_rv1"]) < TOL


def test_trainer_epochs_reporting_plateau_checkpoints(cuda, tmp_path, monkeypatch):
    """LDMTrainer.train / train_epoch driver semantics (reference train.py:210-293): epoch averages times
    config['training_iteration_noise'] (= 50, the reference's reporting multiplier), ReduceLROnPlateau fed
    the epoch loss, ldm_{epoch}.pth written every 100 epochs (epoch 0 here) and loadable weights-only."""
    import models.model as M
    import models.train as TR
    from models.config import config
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").to(cuda)
    ldm.feature_loss_net = _ZeroFeat()
    for p in ldm.encoder.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    batches = [((torch.rand(2, 1, 128, 128, generator=g), torch.zeros(2)),
                (torch.rand(2, 1, 128, 128, generator=g), torch.zeros(2))) for _ in range(3)]
    tr = TR.LDMTrainer(ldm, batches, cuda, lr=1e-3)
    tr.scheduler.patience = 0                    # let the plateau rule fire within 3 epochs
    seen = []
    step = tr.train_step

    def spy(c, s, t=None, noise=None):
        out = step(c, s, t, noise)
        seen.append(out)
        return out

    tr.train_step = spy
    losses, comp, den, sty = tr.train(3)
    k = config["training_iteration_noise"]
    assert k == 50 and len(losses) == 3 and len(seen) == 9
    for e in range(3):
        ep = seen[3 * e: 3 * e + 3]
        assert losses[e] == pytest.approx(sum(o["total_loss"] for o in ep) / 3 * k, rel=1e-6)
        assert den[e] == pytest.approx(sum(o["denoisinsg_loss"] for o in ep) / 3 * k, rel=1e-6)
        assert comp[e] == pytest.approx(sum(o["compression_loss"] for o in ep) / 3 * k, rel=1e-6)
    assert ldm.training
    # plateau: the LR halves whenever the epoch loss did not improve (patience 0)
    lr_expect = 1e-3
    best = float("inf")
    for e in range(3):
        if losses[e] < best * (1 - 1e-4):
            best = losses[e]
        else:
            lr_expect *= 0.5
    assert tr.optimizer.param_groups[0]["lr"] == pytest.approx(lr_expect)
    ck = tmp_path / "models" / "pretrained" / "ldm_0.pth"
    assert ck.exists() and not (tmp_path / "models" / "pretrained" / "ldm_1.pth").exists()
    sd = torch.load(str(ck), map_location="cpu", weights_only=True)
    assert set(sd) == set(ldm.state_dict())


# ---- tap-shared weight gradient (csrc/wgrad.hip) at the train step's shapes --------------------------
# (B, Cin, Hin, Win, Cout, k, stride, pad, out_pad, transposed): one case per kernel instance / chunk form
WGRAD_CASES = {
    "style_enc2_k3s2_rowseg": (2, 64, 64, 256, 128, 3, 2, 1, 0, False),       # <2,3,64,32>, 64-wide segments
    "unet_enc1_k3s1": (2, 32, 16, 64, 64, 3, 1, 1, 0, False),                 # <1,3,64,32>
    "unet_dec1_k3s1_m32": (2, 64, 16, 64, 32, 3, 1, 1, 0, False),             # <1,3,32,32>
    "unet_bottleneck_small_image": (2, 512, 2, 8, 512, 3, 1, 1, 0, False),    # one zero-padded chunk / sample
    "unet_dec4_convT": (2, 512, 2, 8, 256, 3, 2, 1, 1, True),                 # <2,3,64,32> on the input grid
    "unet_dec2_convT_rows": (2, 128, 8, 32, 64, 3, 2, 1, 1, True),            # 2 whole rows per chunk
    "vae_dec0_convT_k4_m32": (2, 32, 16, 64, 128, 4, 2, 1, 0, True),          # <2,4,64,16>, M < BM
    "vae_dec2_convT_k4_c1": (1, 64, 64, 256, 1, 4, 2, 1, 0, True),            # C = 1
    "style_enc1_cin1": (1, 1, 128, 512, 64, 3, 2, 1, 0, False),               # <2,3,64,16>, C = 1
    "style_enc6_k3s2": (2, 256, 4, 16, 512, 3, 2, 1, 0, False),
    "k3s1_c8_b3": (3, 8, 16, 32, 24, 3, 1, 1, 0, False),                      # <1,3,64,16>, M, C ragged
}


@pytest.mark.parametrize("case", sorted(WGRAD_CASES))
def test_wgrad_tap_shared(cuda, case):
    """dW of ldm_conv_backward_weight against float64 torch autograd (1e-5 rel: fp32 MFMA sums over
    K = B*Hq*Wq in split order), twice bitwise equal, and accumulate=1 adding onto dW."""
    from ldm_amd import _lib as L, ops
    B, Cin, H, W, Cout, k, s, p, op, tr = WGRAD_CASES[case]
    seed = zlib.crc32(case.encode()) % 1000
    x = _rand((B, Cin, H, W), seed)
    wshape = (Cin, Cout, k, k) if tr else (Cout, Cin, k, k)
    w = _rand(wshape, seed + 1, -0.2, 0.2)
    xt = torch.from_numpy(x).double()
    wt = torch.from_numpy(w).double().requires_grad_()
    if tr:
        v = tF.conv_transpose2d(xt, wt, None, stride=s, padding=p, output_padding=op)
    else:
        v = tF.conv2d(xt, wt, None, stride=s, padding=p)
    dy = _rand(tuple(v.shape), seed + 5)
    (v * torch.from_numpy(dy).double()).sum().backward()
    desc = ops.make_desc(B, Cin, H, W, Cout, k, k, s, p, op, tr)
    assert int(L.load().ldm_conv_wgrad_workspace_floats(ctypes.byref(desc))) > 0
    xg, dyg = T(x, cuda), T(dy, cuda)
    dw1 = ops.conv_backward_weight(xg, dyg, desc)
    dw2 = ops.conv_backward_weight(xg, dyg, desc)
    torch.cuda.synchronize()
    assert torch.equal(dw1, dw2)
    assert rel_err(npy(dw1), wt.grad.numpy()) < 1e-5
    acc = torch.ones_like(dw1)
    ops.conv_backward_weight(xg, dyg, desc, dw=acc, accumulate=True)
    assert rel_err(npy(acc), wt.grad.numpy() + 1.0) < 1e-5


@pytest.mark.parametrize("shape", [(32, 128, 1, 1), (32, 512, 2, 8), (3, 8, 36, 36), (2, 64, 5, 5),
                                   (4, 96, 8, 8), (5, 24, 8, 16), (3, 40, 16, 16), (2, 8, 16, 32), (2, 16, 16, 64),
                                   (70, 4, 8, 8), (300, 2, 4, 16), (40, 3, 40, 40), (3, 8, 30, 30)])
@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
def test_act_backward_sums(cuda, shape, act):
    """ldm_act_backward (dv, dbias, dbcast) against fp64 on the small-plane kernel (HW <= 16), the multi-plane
    kernel (HW = 64..1024, powers of two: 16-256 threads per plane) and the sliced one (scalar: HW = 25, float4:
    HW % 8 == 4, 8-wide: HW % 8 == 0)."""
    from ldm_amd import ops
    B, C = shape[0], shape[1]
    v = torch.from_numpy(_rand(shape, 31, -2, 2)).double()
    dy = torch.from_numpy(_rand(shape, 32)).double()
    if act == "gelu":
        a = torch.nn.functional.gelu(v)
        dv_ref = dy * (0.5 * (1 + torch.erf(v / 2 ** 0.5)) + v * torch.exp(-0.5 * v * v) / (2 * 3.141592653589793) ** 0.5)
    elif act == "relu":
        a = torch.relu(v)
        dv_ref = dy * (a > 0)
    else:
        a = v
        dv_ref = dy
    dv, db, dbc = ops.act_backward(dy.float().to(cuda), act, act_out=a.float().to(cuda),
                                   pre_act=v.float().to(cuda) if act == "gelu" else None, need_dv=True,
                                   need_bias=True, need_bcast=True)
    assert rel_err(npy(dv), dv_ref.numpy()) < 1e-5
    assert rel_err(npy(db), dv_ref.sum(dim=(0, 2, 3)).numpy()) < 1e-5
    assert rel_err(npy(dbc).reshape(B, C), dy.sum(dim=(2, 3)).numpy()) < 1e-5


@pytest.mark.parametrize("shape", [(2, 8, 4, 4), (3, 16, 8, 8), (2, 16, 16, 64), (3, 40, 16, 16)])
def test_act_backward_none_separate_dv(cuda, shape):
    """ldm_act_backward through the C ABI with act = none and a dv buffer separate from dy (ldm_capi.h: dv =
    dy * act'(v), 'may alias' dy): dv must be written on every kernel form (small planes, the multi-plane
    kernel at HW = 64..1024, the sliced one), with and without the bias sums."""
    from ldm_amd import _lib as L, ops
    B, C = shape[0], shape[1]
    HW = shape[2] * shape[3]
    dy = torch.from_numpy(_rand(shape, 41)).to(cuda)
    for sums in (False, True):
        dv = torch.full_like(dy, float("nan"))
        db = torch.empty(C, device=cuda) if sums else None
        ws = ops.reduce_workspace(B, C, HW, cuda)
        L.call("ldm_act_backward", dy.data_ptr(), None, None, L.ACT["none"], B, C, HW, dv.data_ptr(),
               None if db is None else db.data_ptr(), None, ws.data_ptr(), ops.stream_handle())
        torch.cuda.synchronize()
        assert torch.equal(dv, dy), (shape, sums)
        if sums:
            assert rel_err(npy(db), dy.double().sum(dim=(0, 2, 3)).cpu().numpy()) < 1e-5


# ---- train_ldm: the reference's LDM entry point (train.py:296-316) ------------------------------------------
def test_train_ldm_entry_point(cuda, tmp_path, monkeypatch):
    """models.train.train_ldm end to end on a tiny on-disk pair dataset, as the reference runs it from its
    models/ directory: `import dataset` for the loaders, SpectrogramPairDataset over PNG label folders and a
    pairing CSV, random 80/20 split, LDM(load_full_model=False) loading encoder.pth / decoder.pth from
    models/pretrained/, LDMTrainer.train for two epochs (ReduceLROnPlateau, the x50 reporting, the epoch-0
    checkpoint).  Checks finite per-epoch losses, the frozen encoder untouched, the decoder trained, and the
    checkpoint's keys."""
    import sys
    from PIL import Image
    import models.model as M
    import models.train as TR
    from models.dataset import SpectrogramPairDataset
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "music-style-transfer-ldm_amd", "models"))
    g = np.random.Generator(np.random.PCG64(21))
    root = tmp_path / "processed_images"
    for k in range(2):
        d = root / f"label{k}"
        d.mkdir(parents=True)
        for i in range(3):
            Image.fromarray(g.integers(0, 256, (128, 128), dtype=np.uint8)).save(d / f"s{i:02d}.png")
    pairs = tmp_path / "pairs.csv"
    SpectrogramPairDataset.generate_pairings(str(root), str(pairs), num_pairs=5)
    torch.manual_seed(0)
    enc = M.SpectrogramEncoder(32)
    dec = M.SpectrogramDecoder(32)
    os.makedirs("models/pretrained")
    torch.save(enc.state_dict(), "models/pretrained/encoder.pth")
    torch.save(dec.state_dict(), "models/pretrained/decoder.pth")
    cfg = dict(TR.config)
    cfg.update(processed_spectograms_dataset_folderpath=str(root), pairing_file_path=str(pairs), batch_size=2,
               num_epochs=2, learning_rate=1e-3, style_loss_weight=0.1)
    captured = {}
    orig_init = TR.LDMTrainer.__init__

    def spy(self, model, *a, **k):
        orig_init(self, model, *a, **k)
        captured["model"] = model
    monkeypatch.setattr(TR.LDMTrainer, "__init__", spy)
    tl, comp, den, sty = TR.train_ldm(cfg, device=cuda)
    assert len(tl) == 2 and all(np.isfinite(tl)) and all(np.isfinite(comp)) and all(np.isfinite(den))
    model = captured["model"]
    # frozen parameters (requires_grad False); its BN running statistics still move, since train_epoch puts
    # the whole model in train mode (reference train.py:212)
    for k, v in enc.named_parameters():
        assert torch.equal(dict(model.encoder.named_parameters())[k].detach().cpu(), v.detach()), k
    assert not torch.equal(model.decoder.state_dict()["decoder.0.weight"].cpu(), dec.state_dict()["decoder.0.weight"])
    ck = torch.load("models/pretrained/ldm_0.pth", map_location="cpu", weights_only=True)
    assert set(ck) == set(model.state_dict())
    assert "dataset" in sys.modules


def test_train_autoencoder_entry_point(cuda, tmp_path, monkeypatch):
    """models.train.train_autoencoder (reference train.py:28-138) end to end: loaders from the reference-style
    `dataset` module (SpectrogramDataset over a PNG folder, 80/20 split), AdamW + ReduceLROnPlateau, train /
    validation passes, best-validation and final checkpoints; the saved encoder / decoder load into the
    reference classes and run (finite compression loss, decoder output in [0, 1])."""
    from PIL import Image
    import models.loss as LS
    import models.model as M
    import models.train as TR
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "music-style-transfer-ldm_amd", "models"))
    g = np.random.Generator(np.random.PCG64(23))
    root = tmp_path / "processed_images"
    for k in range(2):
        d = root / f"label{k}"
        d.mkdir(parents=True)
        for i in range(5):
            Image.fromarray(g.integers(0, 256, (128, 128), dtype=np.uint8)).save(d / f"s{i:02d}.png")
    cfg = dict(TR.config)
    cfg.update(processed_spectograms_dataset_folderpath=str(root), batch_size=4, num_epochs=2, learning_rate=1e-3)
    torch.manual_seed(0)
    train_losses, val_losses = TR.train_autoencoder(cfg, device=cuda)
    assert len(train_losses) == 2 and len(val_losses) == 2
    assert all(np.isfinite(train_losses)) and all(np.isfinite(val_losses))
    enc, dec = M.SpectrogramEncoder(32), M.SpectrogramDecoder(32)
    enc.load_state_dict(torch.load("models/pretrained/encoder.pth", map_location="cpu", weights_only=True))
    dec.load_state_dict(torch.load("models/pretrained/decoder.pth", map_location="cpu", weights_only=True))
    enc, dec = enc.to(cuda).eval(), dec.to(cuda).eval()
    # the final checkpoint holds the last epoch's weights: its eval-mode validation pass is finite and the
    # decoder output is a [0, 1] spectrogram
    x = torch.from_numpy(g.integers(0, 256, (2, 1, 128, 128)).astype(np.float32) / 255).to(cuda)
    with torch.no_grad():
        z = enc(x)
        r = dec(z)
        val = LS.compression_loss(x, r, z, LS.VGGishFeatureLoss()).item()
    assert np.isfinite(val) and float(r.min()) >= 0.0 and float(r.max()) <= 1.0
