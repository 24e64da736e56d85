"""CPU: style mixing's float64 yardstick (tests/stylemix_ref.py) and the host-side rules around it.

The yardstick's weighted-exponential attention is pinned to torch's own multi-head attention with a float attn_mask
of log-weights (1e-10 in float64); its duplicate and removal identities hold to 1e-12; LDM.encode_styles checks its
arguments before anything touches a device; the style-window selection rule and the CLI's new flags."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stylemix_ref as MR      # noqa: E402


def attn_sd(E, seed):
    g = torch.Generator().manual_seed(seed)
    return {"a.multihead_attn.in_proj_weight": torch.randn(3 * E, E, generator=g, dtype=torch.float64) / E ** 0.5,
            "a.multihead_attn.in_proj_bias": torch.randn(3 * E, generator=g, dtype=torch.float64) * 0.1,
            "a.multihead_attn.out_proj.weight": torch.randn(E, E, generator=g, dtype=torch.float64) / E ** 0.5,
            "a.multihead_attn.out_proj.bias": torch.randn(E, generator=g, dtype=torch.float64) * 0.1}


@pytest.mark.parametrize("E,h,w,R", [(64, 2, 4, 1), (64, 2, 4, 3), (128, 1, 3, 2)])
def test_yardstick_attention_is_torch_mha_with_a_float_mask(E, h, w, R):
    B, heads = 2, 4
    sd = attn_sd(E, 3 + R)
    g = torch.Generator().manual_seed(17 * R + E)
    x = torch.randn(B, E, h, w, generator=g, dtype=torch.float64)
    maps = torch.randn(B, R, E, h, w, generator=g, dtype=torch.float64)
    wts = torch.rand(B, R, generator=g, dtype=torch.float64) + 0.1
    s = MR.stack(maps)
    kw = MR.key_weights(wts, B, R, h * w)
    got = MR.cross_attention(sd, "a.", x, s, kw)
    q_in = x.reshape(B, E, h * w).permute(2, 0, 1)
    k_in = s.reshape(B, E, R * h * w).permute(2, 0, 1)
    mask = torch.log(kw)[:, None, None, :].expand(B, heads, h * w, R * h * w).reshape(B * heads, h * w, R * h * w)
    want, _ = F.multi_head_attention_forward(
        q_in, k_in, k_in, E, heads, sd["a.multihead_attn.in_proj_weight"], sd["a.multihead_attn.in_proj_bias"], None,
        None, False, 0.0, sd["a.multihead_attn.out_proj.weight"], sd["a.multihead_attn.out_proj.bias"],
        training=False, need_weights=False, attn_mask=mask)
    want = want.permute(1, 2, 0).reshape(B, E, h, w)
    assert rel_err(got.numpy(), want.numpy()) < 1e-10


def test_yardstick_identities():
    E, h, w, B = 64, 2, 4, 2
    sd = attn_sd(E, 9)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, E, h, w, generator=g, dtype=torch.float64)
    a = torch.randn(B, 1, E, h, w, generator=g, dtype=torch.float64)
    b = torch.randn(B, 1, E, h, w, generator=g, dtype=torch.float64)
    single = MR.cross_attention(sd, "a.", x, a[:, 0])
    # duplicates: R copies with any positive weights are the single style
    dup = MR.cross_attention(sd, "a.", x, MR.stack(torch.cat([a, a, a], 1)), MR.key_weights([0.2, 0.7, 0.1], B, 3, h * w))
    assert rel_err(dup.numpy(), single.numpy()) < 1e-12
    # removal: weight 0 is the mix without that reference, per sample too
    ab_ = torch.cat([a, b], 1)
    zero = MR.cross_attention(sd, "a.", x, MR.stack(ab_), MR.key_weights([1.0, 0.0], B, 2, h * w))
    assert rel_err(zero.numpy(), single.numpy()) < 1e-12
    per = MR.cross_attention(sd, "a.", x, MR.stack(ab_), MR.key_weights([[0.5, 0.5], [1.0, 0.0]], B, 2, h * w))
    both = MR.cross_attention(sd, "a.", x, MR.stack(ab_))
    assert rel_err(per[1].numpy(), single[1].numpy()) < 1e-12
    assert rel_err(per[0].numpy(), both[0].numpy()) < 1e-12
    # R = 1 is the oracle's own attention
    from oracle import ldm_torch_cpu as TC
    assert rel_err(single.numpy(), TC.cross_attention(sd, "a.", x, a[:, 0]).numpy()) < 1e-12


def test_encode_styles_argument_checks():
    """Raised on the host, before the style encoder runs (CPU tensors never reach a kernel here)."""
    import models.model as M
    ldm = M.LDM(32, pretrained_path="")
    specs = torch.zeros(2, 3, 1, 128, 64)
    with pytest.raises(ValueError, match="non-negative"):
        ldm.encode_styles(specs, [0.5, -0.1, 0.6])
    with pytest.raises(ValueError, match="positive"):
        ldm.encode_styles(specs, [[0.5, 0.5, 0.0], [0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="references"):
        ldm.encode_styles(torch.zeros(1, 9, 1, 128, 64))
    with pytest.raises(ValueError):
        ldm.encode_styles(specs, [0.5, 0.5])                 # wrong length
    with pytest.raises(ValueError):
        ldm.encode_styles(torch.zeros(2, 1, 128, 64))        # not 5-D
    with pytest.raises(ValueError):
        ldm.content_style_transfer(torch.zeros(2, 1, 128, 64), torch.zeros(2, 1, 128, 64), style_weights=[1.0])
    w = M.LDM.normalise_style_weights([2.0, 6.0], 2)
    assert w.dtype == torch.float64 and torch.allclose(w, torch.tensor([0.25, 0.75], dtype=torch.float64), atol=0, rtol=0)


def test_style_window_selection_rule():
    from models.transfer import style_window_indices as idx
    assert idx(5, 1) == [0] and idx(1, 1) == [0]
    assert idx(5, 2) == [0, 4]
    assert idx(5, 3) == [0, 2, 4]
    assert idx(4, 3) == [0, 2, 3]          # 1.5 rounds up
    assert idx(10, 4) == [0, 3, 6, 9]
    assert idx(1, 3) == [0, 0, 0]          # a recording with one window: copies (the duplicate identity)
    for Ns in range(1, 12):
        for refs in range(2, 9):
            want = [int(math.floor(i * (Ns - 1) / (refs - 1) + 0.5)) for i in range(refs)]
            got = idx(Ns, refs)
            assert got == want and got[0] == 0 and got[-1] == Ns - 1 and got == sorted(got)
    with pytest.raises(ValueError):
        idx(0, 1)


def test_cli_parsing():
    from models.transfer import parse_args
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "--out", "o.wav"])
    assert a.style == "b.wav" and a.style_weights is None and a.style_refs == 1      # a single file stays a string
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "c.wav", "--style-weights", "0.7", "0.3", "--style-refs",
                    "2", "--solver", "dpmpp2m", "--out", "o.wav"])
    assert a.style == ["b.wav", "c.wav"] and a.style_weights == [0.7, 0.3] and a.style_refs == 2
    with pytest.raises(SystemExit):
        parse_args(["--content", "a.wav", "--style", "b.wav", "c.wav", "--style-weights", "1", "--out", "o.wav"])
    with pytest.raises(SystemExit):
        parse_args(["--content", "a.wav", "--style", "b.wav", "--style-refs", "0", "--out", "o.wav"])


def test_signature_table_has_the_new_entries():
    from ldm_amd import _lib
    for n in ("ldm_attention_folded_keys", "ldm_attention_fold_keys_bias", "ldm_sample", "ldm_sample_workspace_floats"):
        assert n in _lib.SIGNATURES
    fields = [f[0] for f in _lib.SampleArgs._fields_]
    for f in ("S5", "S6", "key_bias5", "key_bias6"):    # the four mix fields
        assert fields.count(f) == 1
