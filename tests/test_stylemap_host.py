"""CPU: the style map's host side.  LDM.style_map_bias (normalisation, pooling to the two attentions' token grids,
token order, the log), its refusals and the engine's / model's / transfer_recording's before anything touches a
device, longform.style_map_windows and morph_map, the CLI flag, and the float64 yardstick tests/stylemap_ref.py pinned
to tests/stylemix_ref.py (position-constant weights) and to torch's multi-head attention with a per-query float mask."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stylemap_ref as PR      # noqa: E402
import stylemix_ref as MR      # noqa: E402

NEG = float("-inf")


def bias(m, H=16, W=16):
    from models.model import LDM
    return LDM.style_map_bias(m, H, W)


# ---- style_map_bias --------------------------------------------------------------------------------------------------
def test_bias_pooling_normalisation_and_token_order():
    """A 16 x 16 latent map of two references: reference 0 weighs 3 on the left 6 columns and 0 elsewhere against a
    constant 1 of reference 1.  Normalised: 0.75 / 0.25 on columns 0..5, 0 / 1 on the rest.  CA2 cells are 4 x 4
    latent positions (a 4 x 4 grid): cell columns 0, 1, 2, 3 hold 4, 2, 0, 0 of the left columns, so reference 0's
    cell means are 0.75, 0.375, 0, 0; CA1 cells are 8 x 8 (a 2 x 2 grid): 6 of 8 and 0 of 8 columns: 0.5625, 0."""
    m = torch.zeros(1, 2, 16, 16)
    m[0, 0, :, :6] = 3.0
    m[0, 1] = 1.0
    rb5, rb6 = bias(m)
    assert tuple(rb5.shape) == (1, 16, 2) and tuple(rb6.shape) == (1, 4, 2) and rb5.dtype == torch.float32
    want5 = torch.tensor([0.75, 0.375, 0.0, 0.0], dtype=torch.float64)
    for row in range(4):
        for col in range(4):
            tok = row * 4 + col                      # row-major, as the UNet flattens z3
            assert rb5[0, tok, 0] == torch.log(want5[col]).float()
            assert rb5[0, tok, 1] == torch.log(1.0 - want5[col]).float()
    want6 = torch.tensor([0.5625, 0.0], dtype=torch.float64)
    for tok in range(4):
        assert rb6[0, tok, 0] == torch.log(want6[tok % 2]).float()
        assert rb6[0, tok, 1] == torch.log(1.0 - want6[tok % 2]).float()
    # a map that varies along the rows instead lands on the token rows: the order is (row, column)
    rb5t, _ = bias(m.transpose(2, 3).contiguous())
    assert torch.equal(rb5t.view(1, 4, 4, 2), rb5.view(1, 4, 4, 2).transpose(1, 2))


def test_spectrogram_resolution_is_the_latent_map_upsampled():
    g = torch.Generator().manual_seed(3)
    m = torch.rand(2, 3, 16, 24, generator=g) + 0.05
    up = m.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)       # [2,3,128,192]
    a5, a6 = bias(m, 16, 24)
    b5, b6 = bias(up, 16, 24)
    assert torch.equal(a5, b5) and torch.equal(a6, b6)
    # against a direct float64 mean over the cells
    p = (m.double() / m.double().sum(1, keepdim=True)).reshape(2, 3, 4, 4, 6, 4).mean(dim=(3, 5))
    want = torch.log(p).permute(0, 2, 3, 1).reshape(2, 24, 3)
    assert rel_err(a5.double().numpy(), want.numpy()) < 1e-6


def test_position_constant_map_is_log_w_at_every_token():
    from models.model import LDM
    w = torch.tensor([[0.2, 0.5, 0.3], [3.0, 1.0, 0.0]], dtype=torch.float64)
    m = w[:, :, None, None].expand(2, 3, 128, 128)
    rb5, rb6 = bias(m)
    logw = torch.log(LDM.normalise_style_weights(w, 3, 2)).float()      # what encode_styles puts into its key biases
    assert torch.equal(rb5, logw[:, None, :].expand(2, 16, 3)) and torch.equal(rb6, logw[:, None, :].expand(2, 4, 3))
    assert rb5[1, 0, 2] == NEG


def test_one_hot_region_gives_minus_inf_only_on_whole_cells():
    """Reference 0 owns latent columns 0..9 of 16, reference 1 the rest: CA2 cell columns 0, 1 are all reference 0's
    (-inf for 1), column 2 is mixed (both finite), column 3 all reference 1's; CA1 cell column 0 is all 0's, 1 mixed."""
    m = torch.zeros(1, 2, 16, 16)
    m[0, 0, :, :10] = 1.0
    m[0, 1, :, 10:] = 1.0
    rb5, rb6 = bias(m)
    g5 = rb5.view(4, 4, 2)
    assert bool((g5[:, :2, 1] == NEG).all()) and bool((g5[:, :2, 0] == 0).all())
    assert bool(torch.isfinite(g5[:, 2]).all()) and bool((g5[:, 2, 0] == math.log(0.5)).all())
    assert bool((g5[:, 3, 0] == NEG).all()) and bool((g5[:, 3, 1] == 0).all())
    g6 = rb6.view(2, 2, 2)
    assert bool((g6[:, 0, 1] == NEG).all()) and bool(torch.isfinite(g6[:, 1]).all())
    assert not bool(torch.isnan(rb5).any()) and not bool((rb5 == float("inf")).any())


def test_style_map_bias_refusals():
    ok = torch.ones(1, 2, 16, 16)
    for bad in (ok[0], torch.ones(1, 2, 16, 8), torch.ones(1, 2, 64, 64), torch.ones(1, 0, 16, 16), "map"):
        with pytest.raises(ValueError, match="style_map must be"):
            bias(bad)
    for v in (-0.5, float("nan"), float("inf")):
        m = ok.clone()
        m[0, 1, 3, 3] = v
        with pytest.raises(ValueError, match="finite and non-negative"):
            bias(m)
    m = ok.clone()
    m[0, :, 5, 7] = 0.0
    with pytest.raises(ValueError, match="positive weight"):
        bias(m)
    with pytest.raises(ValueError, match="multiples of 8"):
        bias(torch.ones(1, 2, 12, 16), 12, 16)


# ---- engine, model and recording refusals ----------------------------------------------------------------------------
def test_engine_layout_and_value_refusals():
    from ldm_amd.engine import UNetEngine as E
    xs = (2, 32, 16, 64)
    b5, b6 = torch.zeros(2, 64, 3), torch.zeros(2, 16, 3)
    for a, b in ((b5, None), (None, b6)):
        with pytest.raises(ValueError, match="go together"):
            E.map_layout_check(xs, 3, a, b)
    for a, b in ((b5[:, :, :2].contiguous(), b6), (b5, torch.zeros(2, 16, 2)), (b5.double(), b6), (b5, b6.half()),
                 (torch.zeros(3, 64, 2).permute(2, 1, 0), b6), (torch.zeros(1, 64, 3), b6), (b5.tolist(), b6)):
        with pytest.raises(ValueError, match="ref_bias[56] must be"):
            E.map_layout_check(xs, 3, a, b)
    with pytest.raises(ValueError, match="R >= 1"):
        E.map_layout_check(xs, 0, b5, b6)
    with pytest.raises(RuntimeError, match="GPU tensor"):       # well-formed, but on the host
        E.map_layout_check(xs, 3, b5, b6)
    E.map_values_check(b5, torch.full_like(b6, NEG))            # finite and -inf pass
    for v in (float("nan"), float("inf")):
        bad = b5.clone()
        bad[1, 7, 2] = v
        with pytest.raises(ValueError, match=r"NaN / \+inf"):
            E.map_values_check(bad, b6)
        with pytest.raises(ValueError, match=r"NaN / \+inf"):
            E.map_values_check(b5, torch.full_like(b6, v))
    assert E.map_refs(torch.zeros(xs), torch.zeros(2, 256, 12, 16), None) == 3


@pytest.fixture(scope="module")
def ldm():
    import models.model as M
    torch.manual_seed(0)
    return M.LDM(32, pretrained_path="").eval()


def test_model_refusals_before_anything_runs(ldm):
    z = torch.zeros(2, 32, 16, 16)
    emb = {"s5": torch.zeros(2, 256, 8, 4), "s6": torch.zeros(2, 512, 4, 2), "refs": 2, "key_bias5": None,
           "key_bias6": None}
    for bad in (torch.ones(2, 3, 16, 16), torch.ones(1, 2, 16, 16), torch.ones(2, 16, 16)):     # R, B, rank
        with pytest.raises(ValueError, match="one map per sample and reference"):
            ldm.style_conditioned_sample(z, emb, steps=2, t_start=99, style_map=bad)
    with pytest.raises(ValueError, match="finite and non-negative"):
        ldm.style_conditioned_sample(z, emb, steps=2, t_start=99, style_map=-torch.ones(2, 2, 16, 16))
    x = torch.zeros(2, 1, 128, 128)
    with pytest.raises(ValueError, match="5-D style_spec"):
        ldm.content_style_transfer(x, x, steps=2, style_map=torch.ones(2, 1, 128, 128))
    spec = torch.zeros(2, 2, 1, 128, 128)
    with pytest.raises(ValueError, match="one map per sample and reference"):
        ldm.content_style_transfer(x, spec, steps=2, style_map=torch.ones(2, 3, 128, 128))
    with pytest.raises(ValueError, match="style_map must be"):
        ldm.content_style_transfer(x, spec, steps=2, style_map=torch.ones(2, 2, 128, 64))
    # a reference dropped by a zero weight leaves its map row out: the rest must still cover every position
    m = torch.zeros(2, 2, 128, 128)
    m[:, 0] = 1.0
    with pytest.raises(ValueError, match="positive weight"):
        ldm.content_style_transfer(x, spec, steps=2, style_map=m, style_weights=[0.0, 1.0])


def test_per_layer_path_refuses_a_style_map():
    import models.model as M
    torch.manual_seed(2)
    ldm4 = M.LDM(4, pretrained_path="").eval()           # a latent width the fused engine does not take
    z = torch.zeros(2, 4, 16, 16)
    emb = {"s5": torch.zeros(2, 256, 4, 4), "s6": torch.zeros(2, 512, 2, 2), "refs": 1, "key_bias5": None,
           "key_bias6": None}
    with pytest.raises(RuntimeError, match="per-layer"):
        ldm4.style_conditioned_sample(z, emb, steps=2, t_start=99, style_map=torch.ones(2, 1, 16, 16))


def test_transfer_recording_refusals(ldm):
    from models.transfer import transfer_recording
    y = torch.zeros(100 * 512)
    T = 101
    kw = dict(frames=64, overlap=16, num_timesteps=4)
    with pytest.raises(ValueError, match="needs a solver"):
        transfer_recording(ldm, y, [y, y], style_map=torch.ones(2, T), **kw)
    with pytest.raises(ValueError, match="style_refs = 1"):
        transfer_recording(ldm, y, [y, y], style_map=torch.ones(2, T), solver="dpmpp2m", style_refs=2, **kw)
    for bad in (torch.ones(3, T), torch.ones(2, T + 1), torch.ones(2, 64, T), torch.ones(T)):
        with pytest.raises(ValueError, match="style_map must be"):
            transfer_recording(ldm, y, [y, y], style_map=bad, solver="dpmpp2m", **kw)
    m = torch.ones(2, T)
    m[:, 40] = 0.0
    with pytest.raises(ValueError, match="positive sum"):
        transfer_recording(ldm, y, [y, y], style_map=m, solver="dpmpp2m", **kw)
    with pytest.raises(ValueError, match="finite and non-negative"):
        transfer_recording(ldm, y, [y, y], style_map=-torch.ones(2, T), solver="dpmpp2m", **kw)


def test_cli_style_morph():
    from models.transfer import parse_args
    base = ["--content", "a.wav", "--out", "o.wav"]
    a = parse_args(base + ["--style", "b.wav", "c.wav", "--solver", "dpmpp2m", "--style-morph"])
    assert a.style_morph and a.style == ["b.wav", "c.wav"]
    assert not parse_args(base + ["--style", "b.wav"]).style_morph
    for argv in (["--style", "b.wav", "--solver", "dpmpp2m", "--style-morph"],
                 ["--style", "b.wav", "c.wav", "--style-morph"],
                 ["--style", "b.wav", "c.wav", "--solver", "ddim", "--style-morph", "--style-refs", "2"]):
        with pytest.raises(SystemExit):
            parse_args(base + argv)


# ---- recordings ------------------------------------------------------------------------------------------------------
def test_style_map_windows_tail_rule_and_alignment():
    from ldm_amd import longform as LF
    R, M, T = 2, 128, 101                      # the two-window plan of the recording tests: windows at 0 and 48
    g = torch.Generator().manual_seed(5)
    m = torch.rand(R, M, T, generator=g, dtype=torch.float64) + 0.1
    w = LF.style_map_windows(m, 64, 16)
    N, stride = LF.window_plan(T, 64, 16)
    assert (N, stride) == (2, 48) and tuple(w.shape) == (2, R, M, 64) and w.dtype == torch.float64
    assert torch.equal(w[0], m[:, :, 0:64])
    assert torch.equal(w[1, :, :, :T - 48], m[:, :, 48:T])
    assert torch.equal(w[1, :, :, T - 48:], m[:, :, T - 1:T].expand(R, M, 64 - (T - 48)))    # the tail repeats
    # the same cut as the content's and the keep mask's windows wherever frames are real
    for r in range(R):
        k = LF.mask_windows(m[r], 64, 16)
        assert torch.equal(k[0, 0], w[0, r]) and torch.equal(k[1, 0, :, :T - 48], w[1, r, :, :T - 48])
        assert bool((k[1, 0, :, T - 48:] == 0).all())         # where the mask pads zeros, the map must not
    assert bool((w.sum(1) > 0).all())
    # [R, T]: broadcast over the mel bins
    w2 = LF.style_map_windows(m[:, 0], 64, 16, n_mels=128)
    assert tuple(w2.shape) == (2, R, 128, 64) and torch.equal(w2, w2[:, :, :1].expand_as(w2))
    assert torch.equal(w2[:, :, 0], LF.style_map_windows(m[:, :1], 64, 16)[:, :, 0])
    # a single window shorter than the plan's frames
    w3 = LF.style_map_windows(m[:, :, :10], 64, 0)
    assert tuple(w3.shape) == (1, R, M, 64) and torch.equal(w3[0, :, :, 9:], m[:, :, 9:10].expand(R, M, 55))
    with pytest.raises(ValueError):
        LF.style_map_windows(torch.ones(T), 64, 16)
    with pytest.raises(ValueError):
        LF.style_map_windows(m, 60, 16)


@pytest.mark.parametrize("R,T", [(2, 101), (3, 7), (4, 1000), (1, 5), (3, 1), (2, 2)])
def test_morph_map(R, T):
    from ldm_amd import longform as LF
    w = LF.morph_map(R, T)
    assert tuple(w.shape) == (R, T) and w.dtype == torch.float64 and bool((w >= 0).all())
    assert float((w.sum(0) - 1).abs().max()) < 1e-15
    first = torch.zeros(R, dtype=torch.float64)
    first[0] = 1
    assert torch.equal(w[:, 0], first)
    if T > 1:
        assert torch.equal(w[:, -1], first.flip(0))
    if R == 3 and T == 7:       # knots at frames 0, 3, 6
        assert torch.equal(w[:, 3], torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
        assert float((w[:, 1] - torch.tensor([2 / 3, 1 / 3, 0.0], dtype=torch.float64)).abs().max()) < 1e-15
    with pytest.raises(ValueError):
        LF.morph_map(0, 5)


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def attn_sd(E, seed):
    g = torch.Generator().manual_seed(seed)
    return {"a.multihead_attn.in_proj_weight": torch.randn(3 * E, E, generator=g, dtype=torch.float64) / E ** 0.5,
            "a.multihead_attn.in_proj_bias": torch.randn(3 * E, generator=g, dtype=torch.float64) * 0.1,
            "a.multihead_attn.out_proj.weight": torch.randn(E, E, generator=g, dtype=torch.float64) / E ** 0.5,
            "a.multihead_attn.out_proj.bias": torch.randn(E, generator=g, dtype=torch.float64) * 0.1}


def test_yardstick_is_torch_mha_with_a_per_query_mask_and_reduces_to_the_mix():
    B, E, h, w, R, heads = 2, 64, 2, 4, 3, 4
    L, S = h * w, R * h * w
    sd = attn_sd(E, 4)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, E, h, w, generator=g, dtype=torch.float64)
    s = MR.stack(torch.randn(B, R, E, h, w, generator=g, dtype=torch.float64))
    kw = MR.key_weights(torch.rand(B, R, generator=g, dtype=torch.float64) + 0.1, B, R, L)
    rw = torch.rand(B, L, R, generator=g, dtype=torch.float64) + 0.05
    W = PR.pair_weights(B, L, S, kw, rw)
    assert tuple(W.shape) == (B, L, S) and W[1, 3, L + 2] == kw[1, L + 2] * rw[1, 3, 1]
    got = PR.cross_attention(sd, "a.", x, s, W)
    mask = torch.log(W)[:, None].expand(B, heads, L, S).reshape(B * heads, L, S)
    q_in, k_in = x.reshape(B, E, L).permute(2, 0, 1), s.reshape(B, E, S).permute(2, 0, 1)
    want, _ = F.multi_head_attention_forward(
        q_in, k_in, k_in, E, heads, sd["a.multihead_attn.in_proj_weight"], sd["a.multihead_attn.in_proj_bias"], None,
        None, False, 0.0, sd["a.multihead_attn.out_proj.weight"], sd["a.multihead_attn.out_proj.bias"],
        training=False, need_weights=False, attn_mask=mask)
    assert rel_err(got.numpy(), want.permute(1, 2, 0).reshape(B, E, h, w).numpy()) < 1e-10
    # position-constant reference weights are the mix's key weights
    c = torch.rand(B, R, dtype=torch.float64, generator=g) + 0.1
    Wc = PR.pair_weights(B, L, S, None, c[:, None, :].expand(B, L, R))
    a = PR.cross_attention(sd, "a.", x, s, Wc)
    b = MR.cross_attention(sd, "a.", x, s, MR.key_weights(c, B, R, L))
    assert rel_err(a.numpy(), b.numpy()) < 1e-12
    # weight 0 at a query removes the reference there and nowhere else; a query without any key gives 0
    rz = rw.clone()
    rz[1, 1::2, 0] = 0.0
    out = PR.cross_attention(sd, "a.", x, s, PR.pair_weights(B, L, S, kw, rz))
    gone = PR.cross_attention(sd, "a.", x, s[:, :, h:], PR.pair_weights(B, L, S - L, kw[:, L:], rz[:, :, 1:]))
    full = PR.cross_attention(sd, "a.", x, s, PR.pair_weights(B, L, S, kw, rw))
    o, gn, fl = (t.reshape(B, E, L) for t in (out, gone, full))
    assert rel_err(o[1, :, 1::2].numpy(), gn[1, :, 1::2].numpy()) < 1e-12
    assert rel_err(o[1, :, 0::2].numpy(), fl[1, :, 0::2].numpy()) < 1e-12 and rel_err(o[0].numpy(), fl[0].numpy()) < 1e-12
    q = torch.randn(1, 1, 2, 8, dtype=torch.float64, generator=g)
    k = torch.randn(1, 1, 3, 8, dtype=torch.float64, generator=g)
    Wz = torch.tensor([[[1.0, 2.0, 0.5], [0.0, 0.0, 0.0]]], dtype=torch.float64)
    z = PR.attention(q, k, k, Wz)
    assert bool((z[0, 0, 1] == 0).all()) and bool(torch.isfinite(z).all()) and float(z[0, 0, 0].abs().max()) > 0
