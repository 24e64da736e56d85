"""GPU: the style map (per-position style weights), from the reference-bias form of the key-tiled folded attention
(csrc/stylemix.hip) up to transfer_recording, against the float64 yardstick tests/stylemap_ref.py (weighted sums of
exponentials with per-(query, key) weights, written from the definition).

Bars, as tests/test_gpu_stylemix.py's: ATT_TOL = 1e-5 relative for the attention alone, PARITY_TOL = 1e-4 for a loop's
final x against the yardstick and UPD_TOL = 1e-5 for the float64 replay of the coefficient table from the logged eps."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR       # noqa: E402
import regional_ref as RR    # noqa: E402
import solver_ref as SR      # noqa: E402
import stylemap_ref as PR    # noqa: E402
import stylemix_ref as MR    # noqa: E402

pytestmark = pytest.mark.gpu
ATT_TOL, UPD_TOL, PARITY_TOL = 1e-5, 1e-5, 1e-4
NEG = float("-inf")


def npy(t):
    return t.detach().double().cpu().numpy()


# ---- the kernel alone ------------------------------------------------------------------------------------------------
def att_inputs(B, E, L, S, R):
    g = torch.Generator().manual_seed(7 * E + 13 * L + S + R)
    z = torch.randn(B, L, E, generator=g)
    kv = torch.randn(B, 2 * E, S, generator=g)
    wq = torch.randn(E, E, generator=g) / E ** 0.5
    bq = torch.randn(E, generator=g) * 0.1
    kb = torch.randn(B, S, generator=g)
    rb = torch.randn(B, L, R, generator=g)
    return z, kv, wq, bq, kb, rb


def att_ref(z, kv, wq, bq, kb=None, rb=None, keep=None):
    """float64: the unfolded attention with pair weights exp(kb[b,s]) exp(rb[b,l,ref(s)]); keep: key indices kept
    (rb then holds the kept references' columns)."""
    B, L, E = z.shape
    heads, d = 4, E // 4
    q = (torch.einsum("oe,ble->blo", wq.double(), z.double()) + bq.double()) * float(np.sqrt(1.0 / d))
    qh = q.view(B, L, heads, d).permute(0, 2, 1, 3)
    K = kv.double()[:, :E].reshape(B, heads, d, -1).permute(0, 1, 3, 2)
    V = kv.double()[:, E:].reshape(B, heads, d, -1).permute(0, 1, 3, 2)
    if keep is not None:
        K, V = K[:, :, keep], V[:, :, keep]
        kb = None if kb is None else kb[:, keep]
    W = PR.pair_weights(B, L, K.shape[2], None if kb is None else torch.exp(kb.double()),
                        None if rb is None else torch.exp(rb.double()))
    return PR.attention(qh, K, V, W).permute(0, 2, 1, 3).reshape(B, L, E)


def run_att(cuda, z, kv, wq, bq, kb=None, rb=None, R=0, Bm=None, entry="map"):
    """fold the keys, then ldm_attention_folded_keys_map (entry "keys": ldm_attention_folded_keys, no reference bias)."""
    from ldm_amd import _lib as L_
    B, L, E = z.shape
    S, heads = kv.shape[2], 4
    st = torch.cuda.current_stream().cuda_stream
    zd, kvd, wqd, bqd = z.to(cuda), kv.to(cuda), wq.to(cuda), bq.to(cuda)
    kbd = None if kb is None else kb.to(cuda).contiguous()
    rbd = None if rb is None else rb.to(cuda).contiguous()
    kf = torch.empty((B, heads, S, E), device=cuda)
    bf = torch.empty((B, heads, S), device=cuda)
    out = torch.full((B, L, E), float("nan"), device=cuda)
    L_.call("ldm_attention_fold_keys", kvd.data_ptr(), wqd.data_ptr(), bqd.data_ptr(), B, E, heads, S,
            float(np.sqrt(1.0 / (E // heads))), kf.data_ptr(), bf.data_ptr(), st)
    kp = None if kbd is None else kbd.data_ptr()
    if entry == "keys":
        assert rb is None
        L_.call("ldm_attention_folded_keys", zd.data_ptr(), kvd.data_ptr(), kf.data_ptr(), bf.data_ptr(), kp,
                out.data_ptr(), B, E, heads, L, S, st)
    else:
        if rbd is not None:
            assert tuple(rbd.shape) == (B if Bm is None else Bm, L, R)
        L_.call("ldm_attention_folded_keys_map", zd.data_ptr(), kvd.data_ptr(), kf.data_ptr(), bf.data_ptr(), kp,
                None if rbd is None else rbd.data_ptr(), R, B if Bm is None else Bm, out.data_ptr(), B, E, heads, L, S, st)
    torch.cuda.synchronize()
    return out


# 34 / 130: a reference boundary inside a 32- / 64-key tile and a ragged last tile; 20: a ragged query tile
ATT_CASES = [(512, 16, 48, 3), (512, 16, 34, 2), (512, 1, 3, 3), (256, 64, 192, 3), (256, 64, 130, 2), (256, 20, 40, 2),
             (256, 4, 12, 3)]


@pytest.mark.parametrize("E,L,S,R", ATT_CASES)
def test_map_attention_vs_float64(cuda, E, L, S, R):
    z, kv, wq, bq, kb, rb = att_inputs(2, E, L, S, R)
    e0 = rel_err(npy(run_att(cuda, z, kv, wq, bq, None, rb, R)), att_ref(z, kv, wq, bq, None, rb).numpy())
    e1 = rel_err(npy(run_att(cuda, z, kv, wq, bq, kb, rb, R)), att_ref(z, kv, wq, bq, kb, rb).numpy())
    print(f"E {E} L {L} S {S} R {R}: reference bias {e0:.2e}, with a key bias {e1:.2e}")
    assert max(e0, e1) < ATT_TOL


@pytest.mark.parametrize("E,L,S,R", [(512, 16, 48, 3), (256, 20, 40, 2), (256, 64, 130, 2)])
def test_per_query_masking_is_removal_at_those_queries(cuda, E, L, S, R):
    z, kv, wq, bq, _, rb = att_inputs(2, E, L, S, R)
    masked = rb.clone()
    masked[1, 1::2, 0] = NEG
    out = run_att(cuda, z, kv, wq, bq, None, masked, R)
    assert bool(torch.isfinite(out).all())
    full = att_ref(z, kv, wq, bq, None, rb)
    gone = att_ref(z, kv, wq, bq, None, rb[:, :, 1:], keep=list(range(S // R, S)))
    e_gone = rel_err(npy(out[1, 1::2]), gone[1, 1::2].numpy()) if L > 1 else 0.0
    e_same = max(rel_err(npy(out[1, 0::2]), full[1, 0::2].numpy()), rel_err(npy(out[0]), full[0].numpy()))
    print(f"E {E} L {L} S {S}: odd queries against removal {e_gone:.2e}, the rest unchanged {e_same:.2e}")
    assert max(e_gone, e_same) < ATT_TOL


@pytest.mark.parametrize("E,L,S,R", [(512, 16, 34, 2), (256, 20, 130, 2)])
def test_row_with_every_reference_masked_is_exactly_zero(cuda, E, L, S, R):
    z, kv, wq, bq, kb, rb = att_inputs(2, E, L, S, R)
    rows = [0, L - 1] if L > 1 else [0]
    rb[1, rows] = NEG
    out = run_att(cuda, z, kv, wq, bq, kb, rb, R)
    assert bool(torch.isfinite(out).all())
    assert bool((out[1, rows] == 0).all())
    live = [l for l in range(L) if l not in rows]
    want = att_ref(z, kv, wq, bq, kb, rb)
    assert rel_err(npy(out[1, live]), want[1, live].numpy()) < ATT_TOL and rel_err(npy(out[0]), want[0].numpy()) < ATT_TOL


@pytest.mark.parametrize("E,L,S,R", [(512, 16, 48, 3), (256, 64, 130, 2), (256, 20, 40, 2)])
def test_position_constant_bias_is_the_key_bias_bitwise(cuda, E, L, S, R):
    z, kv, wq, bq, _, _ = att_inputs(2, E, L, S, R)
    c = torch.randn(2, R, generator=torch.Generator().manual_seed(S))
    c[1, 0] = NEG
    a = run_att(cuda, z, kv, wq, bq, None, c[:, None, :].expand(2, L, R).contiguous(), R)
    b = run_att(cuda, z, kv, wq, bq, c.repeat_interleave(S // R, dim=1), entry="keys")
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_null_bias_is_the_key_bias_entry_bitwise(cuda):
    for E, L, S in ((512, 16, 48), (256, 64, 130), (512, 16, 16), (256, 64, 64)):       # the last two: the resident kernel
        z, kv, wq, bq, kb, _ = att_inputs(2, E, L, S, 1)
        for bias in (None, kb):
            a = run_att(cuda, z, kv, wq, bq, bias, None, 0)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, run_att(cuda, z, kv, wq, bq, bias, entry="keys"))


@pytest.mark.parametrize("E,L,S,R", [(512, 16, 48, 3), (256, 20, 40, 2)])
def test_samples_past_bm_take_no_bias_bitwise(cuda, E, L, S, R):
    z, kv, wq, bq, kb, rb = att_inputs(2, E, L, S, R)
    both = run_att(cuda, z, kv, wq, bq, kb, rb, R)
    first = run_att(cuda, z, kv, wq, bq, kb, rb[:1], R, Bm=1)
    plain = run_att(cuda, z, kv, wq, bq, kb, entry="keys")
    assert torch.equal(first[1], plain[1]) and torch.equal(first[0], both[0])
    assert not torch.equal(both[1], plain[1])


@pytest.mark.parametrize("E,L,S", [(512, 16, 16), (256, 20, 40), (256, 64, 64)])
def test_one_reference_bias_cancels(cuda, E, L, S):
    """R = 1: a bias per query shifts every score of the row alike, so the softmax does not move."""
    z, kv, wq, bq, _, rb = att_inputs(2, E, L, S, 1)
    e = rel_err(npy(run_att(cuda, z, kv, wq, bq, None, rb, 1)), npy(run_att(cuda, z, kv, wq, bq, entry="keys")))
    print(f"E {E} L {L} S {S}, R 1: {e:.2e}")
    assert e < ATT_TOL


def test_map_entry_refusals(cuda):
    from ldm_amd import _lib as L_
    z, kv, wq, bq, _, rb = att_inputs(2, 256, 4, 12, 3)
    with pytest.raises(L_.LDMError, match="multiple"):          # 12 keys are not 5 references
        run_att(cuda, z, kv, wq, bq, None, rb.new_zeros(2, 4, 5), 5)
    with pytest.raises(L_.LDMError, match=r"\[0, B\]"):         # more biased samples than samples
        run_att(cuda, z, kv, wq, bq, None, rb.new_zeros(3, 4, 3), 3, Bm=3)


# ---- the loops -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(cuda):
    """The model (never modified), its float64 state dict and schedule."""
    import models.model as M
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(cuda)
    sd64 = {k: v.detach().double().cpu() for k, v in ldm.state_dict().items()}
    return dict(M=M, ldm=ldm, sd64=sd64, ab=SR.alpha_bar(ldm.num_timesteps))


def cell_weights(m, cell):
    """float64, from the definition: normalise over R, mean over cell x cell latent positions, [B, L, R] row-major."""
    B, R, H, W = m.shape
    p = m.double() / m.double().sum(1, keepdim=True)
    p = p.reshape(B, R, H // cell, cell, W // cell, cell).mean(dim=(3, 5))
    return p.permute(0, 2, 3, 1).reshape(B, (H // cell) * (W // cell), R)


def map_inputs(ctx, B, H, W, R, seed):
    """z, stacked s5 / s6, a random positive latent-resolution map, its biases and the yardstick's pair weights."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 32, H, W, generator=g)
    m5 = torch.rand(B, R, 256, H // 4, W // 4, generator=g)
    m6 = torch.rand(B, R, 512, H // 8, W // 8, generator=g)
    smap = torch.rand(B, R, H, W, generator=g) ** 3 + 0.01          # positive, a few decades of contrast
    rb5, rb6 = ctx["M"].LDM.style_map_bias(smap, H, W)
    L2, L1 = (H // 4) * (W // 4), (H // 8) * (W // 8)
    rw5, rw6 = cell_weights(smap, 4), cell_weights(smap, 8)
    assert rel_err(npy(torch.exp(rb5.double())), rw5.numpy()) < 1e-6       # style_map_bias against the definition
    return dict(z=z, s5=MR.stack(m5).contiguous(), s6=MR.stack(m6).contiguous(), m5=m5, m6=m6, smap=smap, rb5=rb5, rb6=rb6,
                rw5=rw5, rw6=rw6, W5=PR.pair_weights(B, L2, R * L2, None, rw5), W6=PR.pair_weights(B, L1, R * L1, None, rw6))


def run_loop(ctx, cuda, eng, d, times, solver="msolver", split=1, rb=True, kb=None, **kw):
    z = d["z"]
    B, n = z.shape[0], len(times) - 1
    fd = ctx["ldm"].noise_scheduler
    tt = torch.from_numpy(times)
    coef = (fd.multistep_coefs(tt) if solver == "msolver" else fd.reverse_coefs(tt)).to(cuda)
    t_table = tt[:-1].view(n, 1).expand(n, B).contiguous().to(cuda)
    x = z.to(cuda).clone()
    x0l = torch.full((n,) + tuple(z.shape), float("nan"), device=cuda)
    epl = torch.full_like(x0l, float("nan"))
    if rb:
        kw.update(ref_bias5=d["rb5"].to(cuda), ref_bias6=d["rb6"].to(cuda))
    if kb is not None:
        kw.update(key_bias5=kb[0].to(cuda), key_bias6=kb[1].to(cuda))
    with torch.no_grad():
        if solver == "msolver":
            eng.msolver_loop(x, d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, x0l, epl, split=split, **kw)
        else:
            eng.ddim_loop(x, d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, 0.0, x0l, epl, split=split, **kw)
    torch.cuda.synchronize()
    return x, x0l, epl, coef, t_table


def replay_err(z, x, x0l, epl, coef, times):
    """The float64 replay of the multistep table from the logged eps (tests/test_gpu_solver.py's check)."""
    c = coef.double().cpu().numpy()
    xv, prev, worst = npy(z), None, 0.0
    for i in range(len(times) - 1):
        x0 = (xv - c[i, 1] * npy(epl[i])) / c[i, 0]
        xv = c[i, 2] * xv + c[i, 3] * x0 + (c[i, 4] * prev if prev is not None else 0.0)
        worst = max(worst, rel_err(npy(x0l[i]), x0))
        prev = x0
    return max(worst, rel_err(npy(x), xv))


TIMES = SR.sample_times(99, 4)
MAP_CASES = {"B2-16x64-R2": (2, 16, 64, 2), "B2-16x64-R3": (2, 16, 64, 3), "B1-8x8-R3": (1, 8, 8, 3)}


@pytest.fixture(scope="module")
def map_runs(ctx, cuda):
    """Each 2M case once on the default engine, with its yardstick; shared, never modified."""
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    out = {}
    for k, (B, H, W, R) in MAP_CASES.items():
        d = map_inputs(ctx, B, H, W, R, 140 + R + H)
        want, _, _ = PR.sample(ctx["sd64"], ctx["ab"], TIMES, npy(d["z"]), d["s5"], d["s6"], d["W5"], d["W6"])
        out[k] = (d, run_loop(ctx, cuda, eng, d, TIMES), want)
    return out


@pytest.mark.parametrize("case", list(MAP_CASES))
def test_msolver_loop_map(map_runs, case):
    d, (x, x0l, epl, coef, _), want = map_runs[case]
    e_replay, e_ref = replay_err(d["z"], x, x0l, epl, coef, TIMES), rel_err(npy(x), want)
    print(f"{case}: replay {e_replay:.2e}, yardstick {e_ref:.2e}")
    assert e_replay <= UPD_TOL
    assert e_ref <= PARITY_TOL


def test_ddim_loop_map(ctx, cuda, map_runs):
    d = map_runs["B2-16x64-R2"][0]
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x, x0l, epl, _, _ = run_loop(ctx, cuda, eng, d, TIMES, solver="ddim")
    want, _, _ = PR.sample(ctx["sd64"], ctx["ab"], TIMES, npy(d["z"]), d["s5"], d["s6"], d["W5"], d["W6"], solver="ddim")
    e = rel_err(npy(x), want)
    print(f"ddim eta 0, R 2: {e:.2e}")
    assert e <= PARITY_TOL and bool(torch.isfinite(x0l).all()) and bool(torch.isfinite(epl).all())


def test_msolver_loop_map_without_step_kernels(ctx, cuda, map_runs):
    from ldm_amd.engine import UNetEngine
    d, _, want = map_runs["B2-16x64-R2"]
    x, x0l, epl, coef, _ = run_loop(ctx, cuda, UNetEngine(ctx["ldm"].unet, step=0), d, TIMES)
    e_replay, e_ref = replay_err(d["z"], x, x0l, epl, coef, TIMES), rel_err(npy(x), want)
    print(f"step=0, R 2: replay {e_replay:.2e}, yardstick {e_ref:.2e}")
    assert e_replay <= UPD_TOL and e_ref <= PARITY_TOL


def test_fp16_operands(ctx, cuda, map_runs):
    """The fp16 step kernels under a map, held to twice the error of the key-bias mix on the same engine and inputs
    (z, maps, times; the mix weighs the references by the map's mean), each against its own float64 yardstick.
    Measured on an MI355X: map 7.72e-5, key-bias mix 7.63e-5."""
    from ldm_amd.engine import UNetEngine
    d, _, want = map_runs["B2-16x64-R2"]
    eng = UNetEngine(ctx["ldm"].unet, dtype="fp16")
    x, _, _, _, _ = run_loop(ctx, cuda, eng, d, TIMES)
    w = d["rw6"].mean(1)                                                         # [B,R] float64
    kw5, kw6 = MR.key_weights(w, 2, 2, 64), MR.key_weights(w, 2, 2, 16)
    xm, _, _, _, _ = run_loop(ctx, cuda, eng, d, TIMES, rb=False, kb=(torch.log(kw5).float(), torch.log(kw6).float()))
    want_m, _, _ = MR.sample(ctx["sd64"], ctx["ab"], TIMES, npy(d["z"]), d["s5"], d["s6"], kw5, kw6)
    e_map, e_mix = rel_err(npy(x), want), rel_err(npy(xm), want_m)
    print(f"fp16: map {e_map:.3e}, key-bias mix {e_mix:.3e}")
    assert e_map <= 2 * e_mix


def test_map_composes_with_key_biases(ctx, cuda):
    d = map_inputs(ctx, 1, 8, 8, 2, 171)
    w = torch.tensor([[0.8, 0.2]], dtype=torch.float64)
    kw5, kw6 = MR.key_weights(w, 1, 2, 4), MR.key_weights(w, 1, 2, 1)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x, _, _, _, _ = run_loop(ctx, cuda, eng, d, TIMES, kb=(torch.log(kw5).float(), torch.log(kw6).float()))
    W5, W6 = PR.pair_weights(1, 4, 8, kw5, d["rw5"]), PR.pair_weights(1, 1, 2, kw6, d["rw6"])
    want, _, _ = PR.sample(ctx["sd64"], ctx["ab"], TIMES, npy(d["z"]), d["s5"], d["s6"], W5, W6)
    e = rel_err(npy(x), want)
    print(f"map and key biases: {e:.2e}")
    assert e <= PARITY_TOL


def test_guided_loop_with_a_map(ctx, cuda):
    d = map_inputs(ctx, 2, 16, 64, 2, 172)
    g = torch.Generator().manual_seed(173)
    s5b, s6b = torch.rand(2, 256, 8, 16, generator=g), torch.rand(2, 512, 4, 8, generator=g)
    scale = torch.tensor([1.5, 0.6])
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x, x0l, epl, coef, _ = run_loop(ctx, cuda, eng, d, TIMES, base=(s5b.to(cuda), s6b.to(cuda), None, None),
                                    guidance_scale=scale)
    want, _, _ = PR.sample(ctx["sd64"], ctx["ab"], TIMES, npy(d["z"]), d["s5"], d["s6"], d["W5"], d["W6"],
                           base=(s5b, s6b), s=scale.double().numpy())
    e_replay, e = replay_err(d["z"], x, x0l, epl, coef, TIMES), rel_err(npy(x), want)
    print(f"guided, map on the target only: replay {e_replay:.2e}, yardstick {e:.2e}")
    assert e_replay <= UPD_TOL and e <= PARITY_TOL


def test_keep_with_a_map(ctx, cuda):
    d = map_inputs(ctx, 2, 16, 64, 2, 174)
    g = torch.Generator().manual_seed(175)
    z0, n0 = torch.randn(2, 32, 16, 64, generator=g), torch.randn(2, 32, 16, 64, generator=g)
    w = torch.rand(2, 16, 64, generator=g).round()
    w[:, :, 20:28] = 0.5
    coefs = ctx["ldm"].noise_scheduler.keep_coefs(torch.from_numpy(TIMES))
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x, _, _, _, _ = run_loop(ctx, cuda, eng, d, TIMES, keep=(z0, n0, w, coefs))
    want, _, _ = PR.sample(ctx["sd64"], ctx["ab"], TIMES, npy(d["z"]), d["s5"], d["s6"], d["W5"], d["W6"],
                           keep=(npy(z0), npy(n0), npy(w), RR.keep_coefs(ctx["ab"], TIMES)))
    e = rel_err(npy(x), want)
    print(f"keep and map: {e:.2e}")
    assert e <= PARITY_TOL


def test_split_slices_the_map(ctx, cuda):
    d = map_inputs(ctx, 4, 16, 64, 2, 176)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x1, x0l1, epl1, _, _ = run_loop(ctx, cuda, eng, d, TIMES)
    x2, x0l2, epl2, _, _ = run_loop(ctx, cuda, eng, d, TIMES, split=2)
    e = max(rel_err(npy(x2), npy(x1)), rel_err(npy(x0l2), npy(x0l1)), rel_err(npy(epl2), npy(epl1)))
    print(f"map, split 2 against 1: {e:.2e}")
    assert e <= UPD_TOL
    swapped = dict(d, rb5=d["rb5"].flip(0).contiguous(), rb6=d["rb6"].flip(0).contiguous())
    x3, _, _, _, _ = run_loop(ctx, cuda, eng, swapped, TIMES, split=2)
    for b in range(4):      # every sample's result moves with its own map (the chains read their own slices)
        assert not torch.equal(x3[b], x2[b])


def test_engine_refusals(ctx, cuda):
    from ldm_amd.engine import UNetEngine
    d = map_inputs(ctx, 2, 16, 64, 2, 177)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    times = SR.sample_times(99, 2)
    with pytest.raises(RuntimeError, match="folded"):
        run_loop(ctx, cuda, UNetEngine(ctx["ldm"].unet, fold=False), d, times)
    bad = d["rb5"].clone()
    bad[0, 3, 1] = float("nan")
    with pytest.raises(ValueError, match=r"NaN / \+inf"):
        run_loop(ctx, cuda, eng, dict(d, rb5=bad), times)
    with pytest.raises(ValueError, match="ref_bias6 must be"):
        run_loop(ctx, cuda, eng, dict(d, rb6=d["rb6"][:, :, :1].contiguous()), times)
    with pytest.raises(ValueError, match="go together"):
        run_loop(ctx, cuda, eng, d, times, rb=False, ref_bias5=d["rb5"].to(cuda))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        run_loop(ctx, cuda, eng, d, times, rb=False, ref_bias5=d["rb5"], ref_bias6=d["rb6"])


# ---- identities through the model ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specs(cuda):
    g = torch.Generator().manual_seed(61)
    return dict(z=torch.randn(2, 32, 16, 64, generator=g).to(cuda), st=torch.rand(2, 3, 1, 128, 512, generator=g).to(cuda))


def sample3(ctx, z, emb, **kw):
    with torch.no_grad():
        x, _ = ctx["ldm"].style_conditioned_sample(z, emb, steps=3, t_start=99, **kw)
    torch.cuda.synchronize()
    return x


def test_position_constant_map_is_encode_styles_weights_bitwise(ctx, specs):
    ldm = ctx["ldm"]
    for w in (torch.tensor([0.5, 0.2, 0.3], dtype=torch.float64).expand(2, 3),
              torch.tensor([[0.4, 0.6, 0.0], [0.1, 0.2, 0.7]], dtype=torch.float64)):
        with torch.no_grad():
            weighted = ldm.encode_styles(specs["st"], w)
            equal = ldm.encode_styles(specs["st"])
        assert weighted["key_bias5"] is not None and equal["key_bias5"] is None
        smap = w[:, :, None, None].expand(2, 3, 16, 64)
        a = sample3(ctx, specs["z"], equal, style_map=smap)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, sample3(ctx, specs["z"], weighted))
        assert torch.equal(a, sample3(ctx, specs["z"], equal, style_map=smap.repeat_interleave(8, 2).repeat_interleave(8, 3)))


def test_one_hot_map_is_the_single_style(ctx, specs):
    ldm = ctx["ldm"]
    with torch.no_grad():
        emb = ldm.encode_styles(specs["st"][:, :2])
        plain = sample3(ctx, specs["z"], ldm.style_encoder(specs["st"][:, 1]))
    smap = torch.zeros(2, 2, 16, 64)
    smap[:, 1] = 1.0
    x = sample3(ctx, specs["z"], emb, style_map=smap)
    assert bool(torch.isfinite(x).all())
    e = rel_err(npy(x), npy(plain))
    print(f"one-hot map on reference 1 against its plain call: {e:.2e}")
    assert e <= PARITY_TOL


# ---- capture and the prepared phases ---------------------------------------------------------------------------------
def test_graphed_loop_and_set_style_map(ctx, cuda):
    from ldm_amd.engine import GraphedDDIM
    d = map_inputs(ctx, 2, 16, 64, 2, 181)
    d2 = map_inputs(ctx, 2, 16, 64, 2, 182)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    x1, x0l1, epl1, coef, t_table = run_loop(ctx, cuda, eng, d, TIMES)
    with torch.no_grad():
        gd = GraphedDDIM(eng, d["z"].to(cuda), d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, 0.0, logs=True,
                         solver="msolver", ref_bias5=d["rb5"].to(cuda), ref_bias6=d["rb6"].to(cuda))
        a = gd.replay().clone()
        torch.cuda.synchronize()
        launches = gd.prepare_launches
        assert torch.equal(a, x1) and torch.equal(gd.x0_logs, x0l1) and torch.equal(gd.eps_logs, epl1)
        gd.set_style_map(d2["rb5"].to(cuda), d2["rb6"].to(cuda))
        b = gd.replay().clone()
        b0, be = gd.x0_logs.clone(), gd.eps_logs.clone()
        torch.cuda.synchronize()
    assert gd.prepare_launches == launches == 1
    x2, x0l2, epl2, _, _ = run_loop(ctx, cuda, eng, dict(d, rb5=d2["rb5"], rb6=d2["rb6"]), TIMES)
    assert not torch.equal(x2, x1)
    assert torch.equal(b, x2) and torch.equal(b0, x0l2) and torch.equal(be, epl2)
    with pytest.raises(ValueError, match=r"NaN / \+inf"):
        gd.set_style_map(torch.full_like(d2["rb5"], float("inf")).to(cuda), d2["rb6"].to(cuda))
    with torch.no_grad():
        plain = GraphedDDIM(eng, d["z"].to(cuda), d["s5"].to(cuda), d["s6"].to(cuda), t_table, coef, 0.0, solver="msolver")
    with pytest.raises(ValueError, match="without a style map"):
        plain.set_style_map(d["rb5"].to(cuda), d["rb6"].to(cuda))


@pytest.mark.parametrize("solver", ["msolver", "ddim"])
def test_one_prepare_serves_runs_with_other_maps(ctx, cuda, solver):
    """ldm_sample_prepare once, then ldm_sample_run under two different maps: each is the whole ldm_sample, bitwise."""
    from ldm_amd.engine import LoopOptions
    d = map_inputs(ctx, 2, 16, 64, 2, 183)
    d2 = map_inputs(ctx, 2, 16, 64, 2, 184)
    eng = ctx["M"].engine_for(ctx["ldm"].unet)
    slot = ("test", "prepared-map")
    z, s5, s6 = d["z"].to(cuda), d["s5"].to(cuda), d["s6"].to(cuda)
    first = True
    for m in (d, d2):
        x1, x0l1, epl1, coef, t_table = run_loop(ctx, cuda, eng, dict(d, rb5=m["rb5"], rb6=m["rb6"]), TIMES, solver=solver)
        x = z.clone()
        x0l, epl = torch.full_like(x0l1, float("nan")), torch.full_like(epl1, float("nan"))
        opts = LoopOptions(x, t_table.shape[0], s5, s6, ref_bias5=m["rb5"].to(cuda), ref_bias6=m["rb6"].to(cuda))
        opts.check(eng, x, t_table.shape[0])
        args = (solver, x, opts, t_table, coef, 0.0, x0l, epl, 0, slot)
        if first:
            eng._sample_call(*args, phase="prepare")
            first = False
        eng._sample_call(*args, phase="run")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(x1).all())
        assert torch.equal(x, x1) and torch.equal(x0l, x0l1) and torch.equal(epl, epl1)
    eng.release_workspaces(slot)


# ---- the whole recording ---------------------------------------------------------------------------------------------
def test_transfer_recording_with_a_style_map(ctx, cuda):
    from ldm_amd import audio as A
    from ldm_amd import longform as LF
    from models.transfer import transfer_recording
    ldm = ctx["ldm"]
    content = torch.from_numpy(AR.test_signal(100 * 512)).float().to(cuda)     # 101 frames: two windows of 64 / 16
    style = torch.from_numpy(AR.test_signal(200 * 512, variant=1)).float().to(cuda)
    style2 = torch.from_numpy(AR.test_signal(70 * 512, variant=2)).float().to(cuda)
    kw = dict(frames=64, overlap=16, n_iter=2, nnls_iters=2, seed=4, num_timesteps=4, solver="dpmpp2m")
    x, ref = LF.mel_windows(A.melspectrogram(content), 64, 16)
    xs, _ = LF.mel_windows(A.melspectrogram(style), 64, 0)
    xs2, _ = LF.mel_windows(A.melspectrogram(style2), 64, 0)
    spec = torch.cat([xs[:1], xs2[:1]]).unsqueeze(0).expand(2, -1, -1, -1, -1)
    noise = torch.randn((2, 32, 16, 8), generator=torch.Generator().manual_seed(4)).to(cuda)
    smap = torch.rand(2, 128, 101, generator=torch.Generator().manual_seed(9), dtype=torch.float64) + 0.05
    smap[0, :64, :30] = 0.0                                  # low band of the opening: the second recording alone
    res = transfer_recording(ldm, content, [style, style2], style_map=smap, **kw)
    assert res.N == 2
    windows = LF.style_map_windows(smap, 64, 16)
    with torch.no_grad():
        want, _ = ldm.content_style_transfer(x, spec, t_start=99, steps=4, solver="dpmpp2m", noise=noise,
                                             style_map=windows)
        other, _ = ldm.content_style_transfer(x, spec, t_start=99, steps=4, solver="dpmpp2m", noise=noise)
    assert bool(torch.isfinite(want).all()) and torch.equal(res.windows_out, want) and not torch.equal(want, other)
    assert torch.equal(res.mel_power, LF.stitch_windows(want, ref, 16, 101))
    # a position-constant map is the style_weights call
    const = torch.tensor([0.7, 0.3], dtype=torch.float64)[:, None].expand(2, 101)
    a = transfer_recording(ldm, content, [style, style2], style_map=const, **kw)
    b = transfer_recording(ldm, content, [style, style2], style_weights=[0.7, 0.3], **kw)
    assert torch.equal(a.windows_out, b.windows_out) and torch.equal(a.audio, b.audio)
    # the morph runs end to end and differs from the even mix
    c = transfer_recording(ldm, content, [style, style2], style_map=LF.morph_map(2, 101), **kw)
    assert bool(torch.isfinite(c.audio).all()) and not torch.equal(c.windows_out, a.windows_out)
