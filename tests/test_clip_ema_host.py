"""Host side of gradient-norm clipping and EMA weights (no device): the float64 reference module against
hand-worked cases, argument validation, the EMA state dict's key set, the config keys."""
import math

import numpy as np
import pytest
import torch

import clip_ema_ref as R


def test_reference_norm_and_coefficient_by_hand():
    gs = [np.array([3.0], np.float32), np.array([[0.0, 4.0]], np.float32), np.array([12.0], np.float32)]
    assert R.grad_norm(gs) == 13.0                           # sqrt(9 + 16 + 144)
    assert R.clip_coef(13.0, 26.0) == 1.0                    # below max_norm: exactly 1
    assert R.clip_coef(13.0, 6.5) == 6.5 / (13.0 + 1e-6)
    assert R.clip_coef(13.0, 0.0) == 1.0 and R.clip_coef(13.0, -2.0) == 1.0
    assert R.clip_coef(math.inf, 1.0) == 0.0 and math.isnan(R.clip_coef(math.nan, 1.0))
    # the coefficient is torch's
    ps = [torch.nn.Parameter(torch.zeros(g.shape)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_(ps, 6.5)
    assert float(total) == 13.0
    for p, g in zip(ps, gs):
        np.testing.assert_allclose(p.grad.numpy(), g * R.clip_coef(13.0, 6.5), rtol=1e-6)


def test_reference_adam_and_ema_by_hand():
    # first step from zero moments: m = (1-b1) g, v = (1-b2) g^2, so the update is lr * g / (|g| + eps)
    p, m, v = R.adam_step([1.0, -2.0], [0.5, -0.25], [0.0, 0.0], [0.0, 0.0], 1, lr=0.1, eps=0.0)
    np.testing.assert_allclose(p, [0.9, -1.9], rtol=1e-12)
    np.testing.assert_allclose(m, [0.05, -0.025], rtol=1e-12)
    np.testing.assert_allclose(v, [0.00025, 0.0000625], rtol=1e-12)
    # a clip coefficient scales the gradient before everything else
    p2, m2, _ = R.adam_step([1.0], [4.0], [0.0], [0.0], 1, lr=0.1, eps=0.0, coef=0.25)
    np.testing.assert_allclose(m2, [0.1], rtol=1e-12)
    # AdamW decays the parameter first; Adam adds wd * p to the gradient
    pw, _, _ = R.adam_step([2.0], [1.0], [0.0], [0.0], 1, lr=0.1, eps=0.0, weight_decay=0.5, decoupled=True)
    np.testing.assert_allclose(pw, [2.0 * 0.95 - 0.1], rtol=1e-12)
    _, ml, _ = R.adam_step([2.0], [1.0], [0.0], [0.0], 1, lr=0.1, eps=0.0, weight_decay=0.5)
    np.testing.assert_allclose(ml, [0.1 * 2.0], rtol=1e-12)
    np.testing.assert_allclose(R.ema_step([1.0, 0.0], [2.0, 4.0], 0.9), [1.1, 0.4], rtol=1e-12)
    # three steps against torch.optim.AdamW in float64
    q = torch.nn.Parameter(torch.tensor([0.3, -0.7, 1.1], dtype=torch.float64))
    opt = torch.optim.AdamW([q], lr=1e-2, weight_decay=0.1)
    pn, mn, vn = q.detach().numpy().copy(), np.zeros(3), np.zeros(3)
    for step in range(1, 4):
        g = np.array([0.2, -0.4, 0.05]) * step
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        pn, mn, vn = R.adam_step(pn, g, mn, vn, step, lr=1e-2, weight_decay=0.1, decoupled=True)
    np.testing.assert_allclose(pn, q.detach().numpy(), rtol=1e-12)


def test_reference_tensor_set_reaches_every_chunk_path():
    n = [int(np.prod(s)) for s in R.SHAPES]
    assert {1, 3, 4096, 4097, 4098, 12289, 35} <= set(n)
    gs = R.grads(5)
    big = np.abs(gs[R.BIG_INDEX]).mean()
    assert all(big > 300 * np.abs(g).mean() for i, g in enumerate(gs) if i != R.BIG_INDEX and g.size > 100)
    assert R.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1


@pytest.mark.parametrize("decay", [-0.1, 1.0, 1.5, float("nan"), "0.9", True])
def test_attach_ema_rejects_bad_decay(decay):
    from ldm_amd import optim as hoptim
    opt = hoptim.Adam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="EMA decay"):
        opt.attach_ema(decay)
    assert opt.ema_decay is None and len(opt.state) == 0


def test_attach_ema_twice_raises_and_state_carries_the_ema():
    from ldm_amd import optim as hoptim
    p = torch.nn.Parameter(torch.arange(4.0))
    opt = hoptim.AdamW([p])
    opt.attach_ema(0.0)                # the bounds are inclusive below
    with pytest.raises(RuntimeError, match="already"):
        opt.attach_ema(0.5)
    assert opt.ema_decay == 0.0
    e = opt.state[p]["ema"]
    assert torch.equal(e, p.detach()) and e.data_ptr() != p.data_ptr()
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"ema"}
    # loading a state dict without the key re-initialises the EMA from the parameters
    with torch.no_grad():
        p.add_(1.0)
    opt.load_state_dict({"state": {}, "param_groups": sd["param_groups"]})
    assert torch.equal(opt.state[p]["ema"], p.detach())


def test_ema_update_rejects_bad_decay():
    from ldm_amd import optim as hoptim
    with pytest.raises(ValueError, match="EMA decay"):
        hoptim.ema_update_([torch.zeros(3)], [torch.zeros(3)], 1.0)


def test_trainer_ema_state_dict_key_set():
    import models.model as M
    import models.train as TR
    m = M.LDM(32, pretrained_path="")
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    tr = TR.LDMTrainer(m, [], torch.device("cpu"), ema_decay=0.99, max_grad_norm=1.0)
    assert tr.max_grad_norm == 1.0 and tr.ema_decay == 0.99 and tr.last_grad_norm is None
    sd, esd = m.state_dict(), tr.ema_state_dict()
    assert list(esd) == list(sd)
    named = dict(m.named_parameters())
    for k, v in esd.items():
        assert torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr(), k       # a copy, equal before any step
    assert {k for k, p in named.items() if p.requires_grad} == \
        {k for k, p in named.items() if "ema" in tr.optimizer.state.get(p, {})}
    assert all("ema" not in tr.optimizer.state.get(named[k], {}) for k in frozen)
    plain = TR.LDMTrainer(M.LDM(32, pretrained_path=""), [], torch.device("cpu"))
    assert plain.max_grad_norm is None and plain.ema_decay is None and plain.last_grad_norm is None
    with pytest.raises(RuntimeError, match="no EMA"):
        plain.ema_state_dict()


def test_config_has_both_keys_off():
    from models.config import config
    assert "max_grad_norm" in config and config["max_grad_norm"] is None
    assert "ema_decay" in config and config["ema_decay"] is None
